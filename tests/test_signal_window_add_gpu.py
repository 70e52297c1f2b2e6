"""-m gpu: psvr_signal_window_add on the MI355X: the kept window that grows run by run.  The crafted cases of tests/signal_window_cases.py go
psvr_bam_store_append_bgzf -> psvr_signal_run (or psvr_signal_run_pos) -> psvr_signal_window_add in pieces of 1 000 compressed bytes, every
run added to one kept window; psvr_signal_window_text at the end must equal the stdout of the command's host route for the file.  Second
adds begin at every residue modulo 16 and around a tile's end; the window survives runs, grows without losing bytes, is emptied by a
restart and left alone by a refused add; psvr_signal_window behind it is what it was."""
import os

import pytest

import signal_device_cases as sc
import signal_mate_cases as mc
import signal_window_cases as wc
import test_signal as ts
from pansvr_amd import signal_step as ss
from pansvr_amd.sort import BamStore
from test_signal_window_gpu import members_of, pieces_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return sc.build("signal_device_check", sc.tmpdir("swag"), False)


def host_text_of(pairs):
    """(text, offsets) of the state-2 pairs among [(state, text)]"""
    host = [t for x, t in pairs if x == 2]
    off = [0]
    for t in host:
        off.append(off[-1] + len(t))
    return b"".join(host), off


def add_run(sig, info, pairs, at, restart=False):
    """the last run added to the kept window; pairs[at:]: what the file's pairs are expected to be.  (the run's pairs, the totals)"""
    n_front = info.first_error if info.first_error >= 0 else info.pairs
    mine = pairs[at:at + n_front]
    assert sig.pairs()["state"][:n_front].tolist() == [x for x, _ in mine]
    blob, off = host_text_of(mine)
    return mine, sig.window_add(blob, off, restart=restart)


@pytest.fixture(scope="module")
def cases(checker):
    """name: (records, summary, [(state, text)], text)"""
    out = {}
    for name, (states, error) in wc.PATTERNS.items():
        recs, front = wc.records(states, error=error)
        s, tab, text = wc.expected(recs, front, sc.tmpdir("swag"), checker)
        out[name] = (recs, s, wc.cut_by_table(text, tab), text)
    return out


@pytest.mark.parametrize("name", sorted(wc.PATTERNS))
def test_every_run_added_to_one_kept_window_gives_the_host_routes_stdout(cases, name):
    recs, s, pairs, text = cases[name]
    members, header = members_of(recs)
    st, sig = BamStore(), ss.Signal(sc.opt_of(s, []))
    try:
        at, runs, n_bytes, n_pairs, n_host = 0, 0, 0, 0, 0
        for k, p in enumerate(pieces_of(members, 1000)):
            assert not p or st.append_bgzf(p, skip=header if k == 0 else 0, n_ref=len(sc.REFS)) == len(p)
            info = sig.run(st)
            mine, w = add_run(sig, info, pairs, at, restart=k == 0)
            runs, at = runs + 1, at + len(mine)
            n_bytes, n_pairs, n_host = n_bytes + sum(len(t) for _, t in mine), n_pairs + sum(x != 0 for x, _ in mine), n_host + sum(x == 2 for x, _ in mine)
            assert (w.n_bytes, w.n_pairs, w.n_host_pairs) == (n_bytes, n_pairs, n_host)
            if info.first_error >= 0:
                break
            st.drop(info.consumed)
        assert at == len(pairs) and sig.window_text() == text and n_bytes == len(text)
        if len(b"".join(recs)) > 5000:
            assert runs > 4
    finally:
        sig.close(), st.close()


# ---- two adds of one file: sized_records' first pairs and its fill pair in front (their text has a chosen length), the other pairs behind
FRONT_PAIRS = 40


@pytest.fixture(scope="module")
def front_bytes():
    """the text of the front with an empty fill"""
    base = wc.sized_records(0)
    return len(wc.host_route(base[:2 * FRONT_PAIRS] + base[-2:], sc.tmpdir("swag"), wc.ISIZE)[0])


def split_file(checker, target, have, front_pairs=FRONT_PAIRS):
    """(front records, the other records, summary, [(state, text)], text): the front's text has `target` bytes"""
    base = wc.sized_records(target - have)
    front, rest = base[:2 * front_pairs] + base[-2:], base[2 * front_pairs:-2]
    s, tab, text = wc.expected(front + rest, front + rest, sc.tmpdir("swag"), checker)
    pairs = wc.cut_by_table(text, tab)
    assert sum(len(t) for _, t in pairs[:front_pairs + 1]) == target
    return front, rest, s, pairs, text


def two_adds(front, rest, s, pairs, text, between=None):
    """the front's run and the rest's run added to one kept window; between(sig, st, first add's info): called between the two"""
    data, header = sc.bam_file(front)
    st, sig = BamStore(), ss.Signal(sc.opt_of(s, []))
    try:
        data = data[:-28]                                                # (without the end marker: more members follow)
        assert st.append_bgzf(data, skip=header, n_ref=len(sc.REFS)) == len(data)
        info = sig.run(st)
        mine, w1 = add_run(sig, info, pairs, 0, restart=True)
        st.drop(info.consumed)
        first = b"".join(t for _, t in mine)
        assert w1.n_bytes == len(first) and sig.window_text() == first == text[:len(first)]
        if between:
            between(sig, st, w1)
        st.append_bgzf(ts.bgzf(b"".join(rest)), n_ref=len(sc.REFS))            # (members of records alone)
        info = sig.run(st)
        more, w2 = add_run(sig, info, pairs, len(mine))
        assert len(mine) + len(more) == len(pairs) and w2.n_bytes == len(text) and w2.n_pairs == sum(x != 0 for x, _ in pairs) and w2.n_host_pairs == sum(x == 2 for x, _ in pairs)
        assert sig.window_text() == text
        return w1, w2
    finally:
        sig.close(), st.close()


@pytest.mark.parametrize("residue", range(16))
def test_a_second_add_begins_at_every_residue(checker, front_bytes, residue):
    target = (front_bytes + 15) // 16 * 16 + 16 + residue
    w1, _ = two_adds(*split_file(checker, target, front_bytes))
    assert w1.n_bytes % 16 == residue


@pytest.mark.parametrize("target", [wc.TILE - 1, wc.TILE, wc.TILE + 1])
def test_a_first_add_ends_around_a_tile(checker, front_bytes, target):
    assert front_bytes < wc.TILE - 1
    w1, w2 = two_adds(*split_file(checker, target, front_bytes))
    assert w1.n_bytes == target and w2.n_bytes > target + 1000


def test_an_add_that_grows_the_buffer_keeps_the_earlier_bytes(checker):
    """three pairs and the fill in front, 77 pairs behind: the second add needs many times the room the first one allocated"""
    base = wc.sized_records(0)
    have = len(wc.host_route(base[:6] + base[-2:], sc.tmpdir("swag"), wc.ISIZE)[0])
    w1, w2 = two_adds(*split_file(checker, have + 5, have, front_pairs=3))
    assert w2.n_bytes > 8 * (w1.n_bytes + 16)


def test_the_kept_window_survives_runs_and_a_refused_add_and_restarts(checker, front_bytes):
    front, rest, s, pairs, text = split_file(checker, front_bytes + 3, front_bytes)
    seen = {}

    def between(sig, st, w1):
        first = sig.window_text()
        for _ in range(2):                                               # runs (over an empty store): the kept window stays
            info = sig.run(st)
            assert info.pairs == 0 and sig.window_text(0, w1.n_bytes) == first
        w = sig.window_add()                                             # an empty run added: nothing changes
        assert (w.n_bytes, w.n_pairs, w.n_host_pairs) == (w1.n_bytes, w1.n_pairs, w1.n_host_pairs) and sig.window_text() == first
        for why, args in (("not the number", (b"x", [0, 1])), ("without a host pair", (b"x", [0])), ("a negative count", (b"", []))):
            with pytest.raises(ss.EngineError, match="psvr error 1: .*" + why):
                sig.window_add(*args)
            assert sig.window_text(0, w1.n_bytes) == first
        with pytest.raises(ss.EngineError, match="psvr error 1"):        # (the totals stand: one byte more is outside the window)
            sig.window_text(0, w1.n_bytes + 1)
        seen["first"] = first

    two_adds(front, rest, s, pairs, text, between)
    assert seen["first"] == text[:front_bytes + 3]
    # restart, and psvr_signal_window behind a kept window
    data, header = sc.bam_file(front + rest)
    st, sig = BamStore(), ss.Signal(sc.opt_of(s, []))
    try:
        st.append_bgzf(data, skip=header, n_ref=len(sc.REFS))
        info = sig.run(st)
        _, w = add_run(sig, info, pairs, 0, restart=True)
        _, w = add_run(sig, info, pairs, 0)                              # the same run twice: its window twice
        assert w.n_bytes == 2 * len(text) and w.n_pairs == 2 * sum(x != 0 for x, _ in pairs) and sig.window_text() == text + text
        _, w = add_run(sig, info, pairs, 0, restart=True)
        assert w.n_bytes == len(text) and sig.window_text() == text
        blob, off = host_text_of(pairs)
        w = sig.window(blob, off)                                        # the run's own window: as before, and gone with the next run
        assert (w.n_bytes, w.n_pairs, w.n_host_pairs) == (len(text), info.written + info.declined, info.declined) and sig.window_text() == text
        sig.run(st)
        with pytest.raises(ss.EngineError, match="no window"):
            sig.window_text(0, 1)
        info = sig.info                                                  # (the same records again, STAT_ spent; no kept window any more: the add begins one)
        _, w = add_run(sig, info, pairs, 0)
        assert (w.n_bytes, w.n_pairs) == (info.text_bytes + len(blob), info.written + info.declined) and len(sig.window_text()) == w.n_bytes < len(text)
    finally:
        sig.close(), st.close()


def test_the_blocks_of_a_position_sorted_file_in_one_kept_window():
    """psvr_signal_run_pos and psvr_signal_run_left: the crafted position-sorted file's blocks and its by-name pass, -D (every pair is written,
    none by the host), all in one kept window: the command's host route's stdout"""
    tmp = sc.tmpdir("swag")
    bam = mc.write(os.path.join(tmp, "in.bam"), mc.crafted())
    h, _, _ = mc.run_cmd(mc.CLI, tmp, bam, ["-D", "--isize", "100,300,500", "--block-records", "64"], "h")
    assert h.returncode == 0 and len(h.stdout) > 5000
    read_len = int(h.stdout.split(b"STAT_")[1].split(b"_")[0])
    data, header = sc.bam_file(mc.crafted(), mc.REFS)
    # (isize_min / isize_max as SignalStep::run derives them from --isize)
    st, sig = BamStore(), ss.Signal(ss.signal_opt([read_len, 100, 300, 500], 1, 650, not_use_filter=True))
    try:
        assert st.append_bgzf(data, skip=header, n_ref=len(mc.REFS)) == len(data)
        blocks, w, restart = 0, None, True
        while True:
            info, pi = sig.run_pos(st, finish=True, block_records=64)
            assert pi.complete == 1
            if pi.primaries >= 2:
                assert info.declined == 0 and info.first_error < 0
                w, restart, blocks = sig.window_add(restart=restart), False, blocks + 1
            st.drop(pi.consumed)
            if pi.primaries < 2:
                break
        first = 0
        while True:
            info, li = sig.run_left(first, 5)
            assert info.declined == 0 and info.first_error < 0
            w = sig.window_add()
            if not li.more:
                break
            first += li.n_pairs
        assert blocks > 2 and first > 0 and w.n_bytes == len(h.stdout) and w.n_pairs == h.stdout.count(b"\n") // 8 and w.n_host_pairs == 0
        assert sig.window_text() == h.stdout
    finally:
        sig.close(), st.close()
