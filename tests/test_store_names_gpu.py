"""-m gpu: psvr_bam_store_order_names (pansvr_amd.sort.BamStore.order_names) on the MI355X: a store filled from the host and through append_bgzf,
in small chunks and segments, with the names of tests/name_cases.py (so that the names' addresses take every residue modulo 8), is ordered by
name; the table, the streamed bytes and the download are held to the restatement (Python's sorted() on (name, flag & 0xc0, index), the bin
recomputed as tests/test_bam_store_gpu.py restates it)."""
import numpy as np
import pytest

import bam_stream
import inflate_cases as ic
import name_cases as nc
from test_bam_store_gpu import REFS, check_meta, chunk_bytes, expectation, make_record, streamed
from test_sort_device_gpu import make_store

pytestmark = pytest.mark.gpu

_SETS = {}


def record_set(what):
    """(records, the restated name order, test_bam_store_gpu's expectation) -- made once, shared, never changed"""
    if what not in _SETS:
        g = nc.groups()
        recs = {"cases": lambda: nc.records(g["everything"], seed=2),
                "cases+bulk": lambda: nc.records(g["everything"], seed=4, bare_last=False) + nc.bulk(4 * 2048 + 7 - len(g["everything"]), 21),
                "bulk-2049": lambda: nc.bulk(2049, 22), "one": lambda: nc.records(g["one name"]), "none": lambda: []}[what]()
        _SETS[what] = (recs, nc.restated_order(recs), expectation(recs))
    return _SETS[what]


def hold_by_name(st, recs, order, exp, key_exact=1):
    fixed, _, info = exp
    n = len(recs)
    i = st.info()
    assert (i.n_records, i.n_bytes, i.key_exact, i.ordered) == (n, sum(map(len, recs)), key_exact, 0)
    st.order_names()
    assert st.info().ordered == 2
    meta = st.meta()
    assert meta["index"].tolist() == order
    check_meta(meta, np.array(order, dtype=np.int64), info)
    want = b"".join(fixed[k] for k in order)
    got = streamed(st, n, 3000, 2)
    assert got == want, bam_stream.first_difference(b"BAM\1\0\0\0\0\0\0\0\0" + got, b"BAM\1\0\0\0\0\0\0\0\0" + want)
    assert st.download().tobytes() == b"".join(fixed)                           # append order, as before
    st.order_names()                                                            # again: nothing to do
    assert st.info().ordered == 2


@pytest.mark.parametrize("what,chunk,piece", [("none", 0, 1), ("one", 0, 1), ("cases", 4096, 7), ("cases", 0, 1000), ("bulk-2049", 65536, 300), ("cases+bulk", 4096, 50), ("cases+bulk", 0, 100000)])
def test_host_appends_ordered_by_name(what, chunk, piece):
    from pansvr_amd._lib import EngineError
    from pansvr_amd.sort import BamStore
    recs, order, exp = record_set(what)
    with chunk_bytes(chunk):
        st = BamStore()
    for a in range(0, len(recs), piece):
        st.append(b"".join(recs[a:a + piece]))
    if what == "cases":
        residues = set()
        at = 0
        for r in recs:                                                          # (chunks begin on 256-byte boundaries at least: with one chunk these are the addresses mod 8)
            residues.add((at + 36) % 8)
            at += len(r)
        assert residues == set(range(8))
    hold_by_name(st, recs, order, exp)
    with pytest.raises(EngineError, match="psvr error 1"):                      # PSVR_ERR_ARG: ordered, no more records
        st.append(make_record(60, 0, 5, 0, [], 1))
    with pytest.raises(EngineError, match="ordered by name already"):
        st.order()
    st.close()


@pytest.mark.parametrize("what,block,seg,chunk,every", [("cases", 100, 64, 4096, 1), ("cases", 0xff00, 0, 0, 0), ("bulk-2049", 333, 256, 65536, 7), ("cases+bulk", 0xff00, 256, 0, 3),
                                                        ("cases+bulk", 333, 64, 300000, 0)])
def test_members_in_ordered_by_name(what, block, seg, chunk, every):
    recs, order, exp = record_set(what)
    ms = ic.members_of(b"".join(recs), level=1, block=block)
    st = make_store(seg, chunk)
    every = every or len(ms)
    for a in range(0, len(ms), every):
        data = b"".join(ms[a:a + every])
        assert st.append_bgzf(data, n_ref=len(REFS)) == len(data)
    assert st.chain_info().tail_bytes == 0
    hold_by_name(st, recs, order, exp)
    st.close()


def test_a_pending_tail_refuses_and_the_store_stays_as_it_was():
    from pansvr_amd._lib import EngineError
    recs, order, exp = record_set("bulk-2049")
    buf = b"".join(recs)
    st = make_store(64)
    st.append_bgzf(b"".join(ic.members_of(buf[:-9], level=1, block=333)), n_ref=len(REFS))
    assert st.chain_info().tail_bytes == len(recs[-1]) - 9
    with pytest.raises(EngineError, match="truncated BAM stream"):
        st.order_names()
    with pytest.raises(EngineError, match="psvr error 1"):                      # PSVR_ERR_ARG
        st.order_names()
    assert st.info().ordered == 0
    st.append_bgzf(ic.wrap(ic.deflate(buf[-9:]), buf[-9:]))                     # the next call completes the record
    hold_by_name(st, recs, order, exp)
    st.close()


def test_a_position_outside_the_keys_range_is_no_obstacle():
    from pansvr_amd._lib import EngineError
    from pansvr_amd.sort import BamStore
    base = record_set("cases")[0]
    recs = base[:40] + [nc.with_name(make_record(50, 0, 0x7fffffff, 0x40, [], 3), b"abcdefgh1\0")] + base[40:]
    order, exp = nc.restated_order(recs), expectation(recs)
    st = BamStore()
    st.append(b"".join(recs))
    assert st.info().key_exact == 0
    with pytest.raises(EngineError, match="psvr error 2"):                      # PSVR_ERR_UNSUPPORTED: the coordinate order, as before
        st.order()
    hold_by_name(st, recs, order, exp, key_exact=0)
    st.close()
