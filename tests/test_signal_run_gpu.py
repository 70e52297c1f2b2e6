"""-m gpu: psvr_signal_run (pansvr_amd.signal_step.Signal over a pansvr_amd.sort.BamStore) on the MI355X against the dump of the rules checker
(tests/tools/signal_device_check.cpp: the same rules on the host, held to SignalStep::pair) for the same BAM: the per-pair table, the text,
the counts; the two histograms against numpy; a run that starts at a carried record."""
import struct

import numpy as np
import pytest

import signal_device_cases as sc
import test_signal as ts
from pansvr_amd import signal_step as ss
from pansvr_amd.sort import BamStore

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return sc.build("signal_device_check", sc.tmpdir("srg"), False)


def expected(checker, recs, flags, extra=()):
    """(summary, table, text) of the rules checker for a BAM of these records"""
    d = sc.tmpdir("srg")
    sc.write_bam(d + "/in.bam", recs)
    rc, s, err = sc.run_rules(checker, d + "/in.bam", flags + list(extra), d + "/dump")
    assert rc == 0, err[-2000:]
    return s, sc.read_tab(d + "/dump"), open(d + "/dump.fq", "rb").read()


def filled_store(recs, calls=1):
    data, header = sc.bam_file(recs)
    st = BamStore()
    at = 0
    for k in range(calls):
        end = len(data) if k == calls - 1 else at + (len(data) - at) // (calls - k)
        at += st.append_bgzf(data[at:end], skip=header if at == 0 else 0, n_ref=len(sc.REFS))
    assert st.chain_info().tail_bytes == 0 and st.info().n_records == len(recs)
    return st


def check_run(sig, info, tab, text, first=0):
    assert info.pairs == len(tab) and info.text_bytes == len(text)
    assert info.written == sum(t[0] == 1 for t in tab) and info.declined == sum(t[0] == 2 for t in tab) and info.first_error == -1
    got = sig.pairs()
    assert got["state"].tolist() == [t[0] for t in tab] and got["note"].tolist() == [t[1] for t in tab] and got["bytes"].tolist() == [t[2] for t in tab]
    assert got["rec1"].tolist() == [t[3] + first for t in tab] and got["rec2"].tolist() == [t[4] + first for t in tab]
    assert got["text_off"].tolist() == np.concatenate([[0], np.cumsum([t[2] for t in tab])[:-1]]).tolist()
    assert sig.text() == text
    # the side records: both records of every declined or noted pair, back to back in pair order, and of no other
    side, at = sig.side(), 0
    for t, off in zip(tab, got["side_off"].tolist()):
        if t[0] == 2 or t[1]:
            assert off == at
            for k in (3, 4):
                n = 4 + struct.unpack_from("<I", side, at)[0]
                at += n
        else:
            assert off == -1
    assert at == len(side) == info.side_bytes


def histograms(recs, tab):
    a, b = np.zeros(ss.MAX_ISIZE, dtype=np.uint64), np.zeros(ss.MAX_LEN, dtype=np.uint64)
    for t in tab:
        for r in (recs[t[3]], recs[t[4]]):
            l_seq, isize = struct.unpack_from("<i", r, 20)[0], abs(struct.unpack_from("<i", r, 32)[0])
            if 0 < isize < ss.MAX_ISIZE:
                a[isize] += 1
            if l_seq < ss.MAX_LEN:
                b[l_seq] += 1
    return a, b


@pytest.mark.parametrize("flags,seed", sc.FLAG_SETS)
def test_table_text_and_histograms_equal_the_rules_checker(checker, flags, seed):
    recs, _ = ts.make_pairs(seed, 600)
    s, tab, text = expected(checker, recs, flags)
    st, sig = filled_store(recs, calls=3), ss.Signal(sc.opt_of(s, flags))
    try:
        info = sig.run(st)
        check_run(sig, info, tab, text)
        assert info.consumed == len(recs) and info.declined > 0
        # the records of a declined pair as the host formatter gets them
        p = [t[0] for t in tab].index(2)
        assert sig.pair_records(st, p) == recs[tab[p][3]] + recs[tab[p][4]]
        off = int(sig.pairs()["side_off"][p])
        assert sig.side()[off:off + len(recs[tab[p][3]]) + len(recs[tab[p][4]])] == recs[tab[p][3]] + recs[tab[p][4]]
        a, b = sig.stats()
        wa, wb = histograms(recs, tab)
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and b.sum() > 1000
        # a second run of the same object: STAT_ has been spent, the histograms add up
        info2 = sig.run(st)
        assert info2.text_bytes <= info.text_bytes and sig.text().count(b"STAT_") == 0 and text.count(b"STAT_") <= 1
        a2, b2 = sig.stats()
        assert np.array_equal(a2, 2 * wa) and np.array_equal(b2, 2 * wb)
    finally:
        sig.close(), st.close()


def test_crafted_edges_on_the_device(checker):
    recs = [r for _, pair, _ in sc.crafted() for r in pair]
    s, tab, text = expected(checker, recs, [])
    st, sig = filled_store(recs), ss.Signal(sc.opt_of(s, []))
    try:
        check_run(sig, sig.run(st), tab, text)
    finally:
        sig.close(), st.close()


def test_a_run_that_starts_at_a_carried_record_and_an_odd_count(checker):
    flags, seed = ["-D"], 20241
    recs, _ = ts.make_pairs(seed, 600)
    s, tab, _ = expected(checker, recs, flags)
    first = tab[100][3]                                              # read 1 of pair 100
    cut = tab[400][4]                                                # the store ends in front of read 2 of pair 400: a lone last primary
    _, tab2, text2 = expected(checker, recs[first:cut], flags, ["--opt", sc.opt_arg(s)])
    assert len(tab2) == 300
    st, sig = filled_store(recs[:cut]), ss.Signal(sc.opt_of(s, flags))
    try:
        info = sig.run(st, first_record=first)
        check_run(sig, info, tab2, text2, first)
        assert info.consumed == tab[400][3]
        # dropping what was consumed leaves the carried record in front: the next run pairs it with what comes
        st.drop(info.consumed)
        assert st.info().n_records == cut - tab[400][3]
        info = sig.run(st)
        assert info.pairs == 0 and info.consumed == 0 and info.text_bytes == 0
    finally:
        sig.close(), st.close()


@pytest.mark.parametrize("state", [3, 4, 5])
def test_error_pair_ends_the_text_and_the_histograms(checker, state):
    front = [r for _, pair, _ in sc.crafted()[:6] for r in pair]
    recs = front + sc.error_pairs()[state] + front
    s, tab, text = expected(checker, recs, ["-D"])
    st, sig = filled_store(recs), ss.Signal(sc.opt_of(s, ["-D"]))
    try:
        info = sig.run(st)
        assert info.pairs == 13 and info.first_error == 6 and info.written == 6 and info.text_bytes == len(text) and sig.text() == text
        got = sig.pairs()
        assert got["state"][:7].tolist() == [t[0] for t in tab] and got["state"][6] == state and got["bytes"][6:].sum() == 0
        _, b = sig.stats()
        assert b.sum() == 12
        err = sc.error_pairs()[state]
        assert got["side_off"][6] >= 0 and sig.side()[int(got["side_off"][6]):] == err[0] + err[1]
    finally:
        sig.close(), st.close()


def test_refusals():
    recs, _ = ts.make_pairs(5, 20)
    st = filled_store(recs)
    sig = ss.Signal(ss.signal_opt([100, 1, 2, 3], 1, 500))
    try:
        for first in (-1, len(recs) + 1):
            with pytest.raises(ss.EngineError, match="first record"):
                sig.run(st, first_record=first)
        with pytest.raises(ss.EngineError, match="no run"):
            sig.pairs()
        sig.run(st)
        st.drop(2)
        with pytest.raises(ss.EngineError, match="dropped"):
            sig.pair_records(st, 0)
        st.order()
        with pytest.raises(ss.EngineError, match="ordered"):
            sig.run(st)
    finally:
        sig.close(), st.close()
