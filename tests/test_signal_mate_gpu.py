"""-m gpu: psvr_signal_run_pos, psvr_signal_mate_notes, psvr_signal_left, psvr_signal_run_left and psvr_signal_left_errors
(pansvr_amd.signal_step.Signal over a pansvr_amd.sort.BamStore) on the MI355X against the host build of the rules: the route checker
(tests/tools/signal_pos_route_check.cpp, held to SignalStep::run_pos_sorted by tests/test_signal_pos_route.py) dumps what every call of a
run over the file answered, and the same calls on the device must answer the same: counts, the pair table with its states, notes, bytes and
offsets, the text, the side records, the unmated records in order, the notes; in phase 2 the order of the left store, the pairing errors in
front of every pair, and slices of 1 and of 3 pairs.  The store is dropped behind every block and has chunks smaller than a block."""
import os
import subprocess

import numpy as np
import pytest

import signal_mate_cases as mc
from pansvr_amd import signal_step as ss
from pansvr_amd.sort import BamStore

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return mc.build("signal_pos_route_check", mc.sc.tmpdir("smg"))


def expected(checker, recs, block, status=0):
    """(options, [call]) of the route checker's dump: call = dict(kind, head, info, pairs, notes, text, side, left)"""
    d = mc.sc.tmpdir("smg")
    mc.write(d + "/in.bam", recs)
    env = dict(os.environ, PSVR_CHECK_DUMP=d + "/dump")
    r = subprocess.run([checker, "signal", "-D", "--mate-device", "-H", d + "/h.sam", "-S", d + "/s.txt"] + (["--block-records", str(block)] if block else []) + [d + "/in.bam"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert r.returncode == status and b" failed (" not in r.stderr, r.stderr[-2000:]
    opt, calls = None, []
    for l in open(d + "/dump.calls", "rb"):
        w = l.split()
        if w[0] == b"O":
            opt = [int(x) for x in w[1:]]
        elif w[0] in (b"B", b"L"):
            k = len(calls)
            blob = lambda what: open("%s/dump.%d.%s" % (d, k, what), "rb").read()
            calls.append(dict(kind=w[0], head=[int(x) for x in w[1:]], pairs=[], notes=[], text=blob("text"), side=blob("side"), left=blob("left")))
        elif w[0] == b"I":
            calls[-1]["info"] = [int(x) for x in w[1:]]
        elif w[0] == b"P":
            calls[-1]["pairs"].append([int(x) for x in w[1:]])
        elif w[0] == b"N":
            calls[-1]["notes"].append(tuple(int(x) for x in w[1:6]) + (w[6],))
    return opt, calls


def same_run(sig, info, c):
    """info, table, text and side records of the last run against a dumped call; returns the table"""
    assert [info.pairs, info.written, info.declined, info.first_error, info.text_bytes, info.side_bytes] == c["info"]
    got = sig.pairs()
    want = np.array(c["pairs"], dtype=np.int64).reshape(-1, 8)
    for k, f in enumerate(("state", "note", "bytes", "rec1", "rec2", "side_off", "text_off")):
        assert got[f].astype(np.int64).tolist() == want[:, k].tolist(), f
    assert sig.text() == c["text"] and sig.side() == c["side"]
    return want


def run_blocks(recs, opt, calls, block, monkeypatch):
    monkeypatch.setenv("PSVR_BAM_STORE_CHUNK_BYTES", "4096")
    monkeypatch.setenv("PSVR_BAM_STORE_SEG_BYTES", "4096")
    data, header = mc.sc.bam_file(recs, mc.REFS)
    o = ss.SignalOpt(*opt[:11])
    for k in range(4):
        o.stat[k] = opt[11 + k]
    st, sig = BamStore(), ss.Signal(o)
    try:
        at, calls_n = 0, 3                                              # three appends: the left-overs of a block lie in several chunks
        for k in range(calls_n):
            end = len(data) if k == calls_n - 1 else at + (len(data) - at) // (calls_n - k)
            at += st.append_bgzf(data[at:end], skip=header if at == 0 else 0, n_ref=len(mc.REFS))
        assert st.chain_info().tail_bytes == 0 and st.info().n_records == len(recs)
        blocks = [c for c in calls if c["kind"] == b"B"]
        for k, c in enumerate(blocks):
            info, pi = sig.run_pos(st, finish=k == len(blocks) - 1, block_records=block or 0)
            assert pi.complete == 1 and [pi.primaries, pi.consumed, pi.unmated, pi.left_bytes, pi.mate_failed, pi.notes, pi.replayed] == c["head"], (k, c["head"])
            same_run(sig, info, c)
            assert sig.left() == c["left"]
            assert [(int(t["number"]), int(t["index"]), int(t["block"]), int(t["tid"]), int(t["pos"]), bytes(t["name"])) for t in sig.mate_notes()] == c["notes"]
            st.drop(pi.consumed)
        info, pi = sig.run_pos(st, finish=True, block_records=block or 0)
        assert pi.complete == 1 and pi.primaries < 2 and info.pairs == 0 and pi.consumed == st.info().n_records
        info, pi = sig.run_pos(st, finish=False, block_records=block or 0)
        assert pi.complete == 0 and pi.consumed == 0
    except BaseException:
        sig.close(), st.close()
        raise
    return st, sig


def run_phase2(sig, calls, max_pairs, text_limit=None):
    """the slices of the device against the dump's (whatever their sizes: the concatenation is one pass); text_limit: the slices are halved
    until their text fits (PSVR_SIGNAL_TEXT_LIMIT is set to it)"""
    want = [c for c in calls if c["kind"] == b"L"]
    w_pairs = [p for c in want for p in c["pairs"]]
    w_text, w_side = b"".join(c["text"] for c in want), b"".join(c["side"] for c in want)
    records, n_pairs, errors = want[0]["head"][:3]
    first_error = next((k for k, p in enumerate(w_pairs) if p[0] >= 3), -1)
    got_pairs, got_errs, text, side, first, at_text, at_side = [], [], b"", b"", 0, 0, 0
    while True:
        info, li = sig.run_left(first, max_pairs)
        assert [li.records, li.pairs, li.errors, li.first_pair] == [records, n_pairs, errors, first] and li.more == (first + li.n_pairs < n_pairs)
        if text_limit is None:
            assert li.n_pairs == min(max_pairs, n_pairs - first)
        else:
            assert 1 <= li.n_pairs <= min(max_pairs, n_pairs - first) and (info.text_bytes <= text_limit or li.n_pairs == 1)
        t = sig.pairs()
        assert info.pairs == li.n_pairs and len(sig.text()) == info.text_bytes
        for p, e in zip(t, sig.left_errors()):
            got_pairs.append([int(p["state"]), int(p["note"]), int(p["bytes"]), int(p["rec1"]), int(p["rec2"]), int(p["side_off"]) + at_side if p["side_off"] >= 0 else -1, int(p["text_off"]) + at_text, int(e)])
        text, side = text + sig.text(), side + sig.side()
        at_text, at_side = len(text), len(side)
        if info.first_error >= 0:
            assert first + info.first_error == first_error
            break
        if not li.more:
            break
        first += li.n_pairs
    # (the dump's offsets are per slice of the checker's run: made running ones the same way)
    w_run, t0, s0 = [], 0, 0
    for c in want:
        for p in c["pairs"]:
            w_run.append(p[:5] + [p[5] + s0 if p[5] >= 0 else -1, p[6] + t0, p[7]])
        t0, s0 = t0 + len(c["text"]), s0 + len(c["side"])
    upto = len(got_pairs)
    if first_error >= 0:                                                # behind the error pair nothing is written: states and records still stand
        assert [p[:2] + p[3:5] for p in got_pairs[:first_error + 1]] == [p[:2] + p[3:5] for p in w_run[:first_error + 1]]
        upto = first_error
    assert [p[:5] + p[7:] for p in got_pairs[:upto]] == [p[:5] + p[7:] for p in w_run[:upto]]
    if first_error < 0:
        assert got_pairs == w_run and text == w_text and side == w_side
    return got_pairs


@pytest.mark.parametrize("block", [None, 3, 64, 65])
def test_crafted_blocks_and_left_overs_equal_the_host_build(checker, monkeypatch, block):
    recs = mc.crafted()
    opt, calls = expected(checker, recs, block)
    assert sum(c["kind"] == b"B" for c in calls) >= 5 and (block or sum(c["head"][6] for c in calls if c["kind"] == b"B") >= 9)
    st, sig = run_blocks(recs, opt, calls, block, monkeypatch)
    try:
        got = run_phase2(sig, calls, block or 1 << 20)
        assert block or (len(got) == 10 and got[-1][7] == 4)            # ten pairs by name; the four pairing errors lie in front of the last
    finally:
        sig.close(), st.close()


@pytest.mark.parametrize("max_pairs", [1, 3])
def test_phase_2_in_slices_of_one_and_of_three_pairs(checker, monkeypatch, max_pairs):
    recs = mc.crafted()
    opt, calls = expected(checker, recs, None)
    st, sig = run_blocks(recs, opt, calls, None, monkeypatch)
    try:
        run_phase2(sig, calls, max_pairs)
    finally:
        sig.close(), st.close()


def test_a_slice_whose_text_would_pass_the_limit_is_halved_until_it_fits(checker, monkeypatch):
    # (the limit is 2 GiB; the test's is 700 bytes, a little more than two pairs of this file)
    recs = mc.crafted()
    opt, calls = expected(checker, recs, None)
    st, sig = run_blocks(recs, opt, calls, None, monkeypatch)
    try:
        monkeypatch.setenv("PSVR_SIGNAL_TEXT_LIMIT", "700")
        sizes = []
        orig = sig.run_left
        sig.run_left = lambda first, m: (lambda r: (sizes.append(r[1].n_pairs), r)[1])(orig(first, m))
        run_phase2(sig, calls, 1 << 20, text_limit=700)
        assert len(sizes) >= 4 and max(sizes) <= 2 and sum(sizes) == 10
    finally:
        sig.close(), st.close()


def test_flags_0x00_and_0xc0_among_equal_names_order_as_the_host_comparator_orders_them(checker, monkeypatch):
    # the record with 0x40 (0xc1) comes first although it lies second in the file; name_tie_key's flag & 0xc0 would have 0x01 first.  The pair
    # is in state 4 (its second record lacks 0x80): the host loop ends there, so the checker's run does, and the slice says where
    rng = np.random.RandomState(8)
    recs = mc.crafted()
    cut = next(k for k, r in enumerate(recs) if r[36:39] == b"tri")
    recs = recs[:cut] + [mc.rec("tie", 0x01, 0, 1500, 3, 5, rng), mc.rec("tie", 0xc1, 0, 1600, 3, 5, rng)] + recs[cut:]
    opt, calls = expected(checker, recs, None, status=34)
    st, sig = run_blocks(recs, opt, calls, None, monkeypatch)
    try:
        got = run_phase2(sig, calls, 1 << 20)
        err = next(p for p in got if p[0] == 4)
        assert err[3] == err[4] + 1                                     # rec1 is the later record of the left store: the one with 0x40
    finally:
        sig.close(), st.close()


def test_every_thousandth_failed_turn_has_its_note(checker, monkeypatch):
    recs = mc.many_failures()
    opt, calls = expected(checker, recs, 2000)
    assert sum(len(c["notes"]) for c in calls) >= 1
    st, sig = run_blocks(recs, opt, calls, 2000, monkeypatch)
    try:
        run_phase2(sig, calls, 2000)
    finally:
        sig.close(), st.close()


def test_what_the_calls_decline(monkeypatch):
    recs = mc.decreasing()
    data, header = mc.sc.bam_file(recs, mc.REFS)
    st, sig = BamStore(), ss.Signal(ss.signal_opt([30, 1, 2, 3], 1, 500))
    try:
        st.append_bgzf(data, skip=header, n_ref=len(mc.REFS))
        with pytest.raises(ss.EngineError, match="positions decrease inside a block"):
            sig.run_pos(st, finish=True)
        assert st.info().n_records == len(recs)
        with pytest.raises(ss.EngineError, match="no block"):
            sig.left()
        sig.left_info = ss.SignalLeftInfo()
        with pytest.raises(ss.EngineError, match="no slice"):
            sig.left_errors()
    finally:
        sig.close(), st.close()


def test_an_odd_number_of_left_overs_is_declined(monkeypatch):
    rng = np.random.RandomState(3)
    recs = [mc.rec("a", 0x61, 0, 100, 0, 200, rng), mc.rec("x", 0x41, 0, 150, 3, 5, rng), mc.rec("a", 0x91, 0, 200, 0, 100, rng), mc.rec("b", 0x41, 0, 300, 3, 5, rng),
            mc.rec("c", 0x41, 0, 400, 3, 5, rng)]
    data, header = mc.sc.bam_file(recs, mc.REFS)
    st, sig = BamStore(), ss.Signal(ss.signal_opt([30, 1, 2, 3], 1, 500, not_use_filter=True))
    try:
        st.append_bgzf(data, skip=header, n_ref=len(mc.REFS))
        info, pi = sig.run_pos(st, finish=True)
        assert pi.primaries == 5 and info.pairs == 1 and pi.unmated == 3
        with pytest.raises(ss.EngineError, match="an odd number of records found no mate"):
            sig.run_left()
    finally:
        sig.close(), st.close()
