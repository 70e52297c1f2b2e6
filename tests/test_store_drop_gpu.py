"""-m gpu: psvr_bam_store_drop and psvr_bam_store_footprint (pansvr_amd.sort.BamStore.drop / footprint) on the MI355X: what stays after a drop,
a pending tail across a drop, order after a drop against Python's sort, the refusals, and the chunks that are released and spared."""
import contextlib
import os
import struct

import pytest

import signal_device_cases as sc
import test_signal as ts
from pansvr_amd.sort import BamStore, EngineError
from test_bam_store_gpu import restate, with_bin

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def pairs():
    recs, _ = ts.make_pairs(31, 300)
    data, header = sc.bam_file(recs)
    return recs, data, header


def fill(st, data, header, calls=3, upto=None):
    """append_bgzf in `calls` calls over data[:upto]; returns the bytes used"""
    n = len(data) if upto is None else upto
    at = 0
    for k in range(calls):
        end = n if k == calls - 1 else at + (n - at) // (calls - k)
        at += st.append_bgzf(data[at:end], skip=header if at == 0 else 0, n_ref=len(sc.REFS))
    return at


def stored(recs):
    """the records as download returns them: the bin recomputed"""
    return b"".join(with_bin(r, restate(r)[5]) for r in recs)


@pytest.mark.parametrize("k", ["0", "1", "n-1", "n"])
def test_drop_leaves_exactly_the_rest(pairs, k):
    recs, data, header = pairs
    n = len(recs)
    k = {"0": 0, "1": 1, "n-1": n - 1, "n": n}[k]
    st = BamStore()
    try:
        fill(st, data, header)
        assert st.info().n_records == n
        st.drop(k)
        i = st.info()
        assert i.n_records == n - k and i.n_bytes == sum(len(r) for r in recs[k:])
        assert st.download().tobytes() == stored(recs[k:])
        st.drop(0)
        assert st.info().n_records == n - k
    finally:
        st.close()


def test_a_pending_tail_stays_pending_across_a_drop(pairs):
    recs, data, header = pairs
    # the members in front of the last one that holds records: the stream they hold ends inside a record
    members, at = [], 0
    while at < len(data):
        members.append(at)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    assert len(members) >= 4                                         # (the EOF block is the last)
    st = BamStore()
    try:
        used = fill(st, data, header, calls=2, upto=members[-2])
        assert used == members[-2]
        have, tail = st.info().n_records, st.chain_info().tail_bytes
        assert 0 < have < len(recs) and tail > 0
        st.drop(have - 1)
        assert st.info().n_records == 1 and st.chain_info().tail_bytes == tail
        with pytest.raises(EngineError, match="only append_bgzf can complete it"):
            st.append(recs[0])
        st.append_bgzf(data[used:])
        assert st.chain_info().tail_bytes == 0 and st.info().n_records == len(recs) - have + 1
        assert st.download().tobytes() == stored(recs[have - 1:])
    finally:
        st.close()


def test_order_after_a_drop_equals_pythons_sort_of_the_rest(pairs):
    recs, data, header = pairs
    st = BamStore()
    try:
        fill(st, data, header)
        st.drop(101)
        rest = recs[101:]
        st.order()
        meta = st.meta()
        want = sorted(range(len(rest)), key=lambda i: (restate(rest[i])[0], i))
        assert meta["index"].tolist() == want
        assert meta["pos"].tolist() == [restate(rest[i])[2] for i in want]
    finally:
        st.close()


def test_refusals(pairs):
    recs, data, header = pairs
    st = BamStore()
    try:
        fill(st, data, header)
        for bad in (-1, len(recs) + 1):
            with pytest.raises(EngineError, match="records of"):
                st.drop(bad)
        assert st.info().n_records == len(recs)
        st.order_names()
        with pytest.raises(EngineError, match="ordered"):
            st.drop(1)
    finally:
        st.close()
    st = BamStore()
    try:
        fill(st, data, header)
        st.order()
        with pytest.raises(EngineError, match="ordered"):
            st.drop(1)
    finally:
        st.close()


def test_footprint_falls_when_small_chunks_empty_and_counts_one_spare(pairs):
    recs, data, header = pairs
    chunk = 80000                                                    # a member inflates to 0xff00 bytes at most: every member's append takes a chunk of its own
    with env(PSVR_BAM_STORE_CHUNK_BYTES=chunk, PSVR_BAM_STORE_SEG_BYTES=4096):
        st = BamStore()
    try:
        assert st.footprint() == (0, 0)
        at, k, peak = 0, 0, 0
        while at < len(data):
            bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
            st.append_bgzf(data[at:at + bsize], skip=header if at == 0 else 0, n_ref=len(sc.REFS))
            at += bsize
            k += 1
            n, b = st.footprint()
            peak = max(peak, n)
            assert b == n * chunk
        assert peak >= 3 and st.info().n_records == len(recs)
        live = st.footprint()[0]
        # everything but the last record goes: the chunk that holds it stays, one of the others is spared
        st.drop(len(recs) - 1)
        n, b = st.footprint()
        assert n == 2 < live and b == 2 * chunk
        assert st.download().tobytes() == stored(recs[-1:])
        # the next chunk the store needs is the spare one: the footprint does not grow
        st.append(recs[0] * (chunk // len(recs[0])))
        assert st.footprint() == (2, 2 * chunk)
        st.drop(st.info().n_records)
        assert st.footprint()[0] <= 2
    finally:
        st.close()
