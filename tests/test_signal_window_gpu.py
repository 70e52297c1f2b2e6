"""-m gpu: psvr_signal_window on the MI355X.  The crafted cases of tests/signal_window_cases.py go psvr_bam_store_append_bgzf -> psvr_signal_run ->
psvr_signal_window; psvr_signal_window_text must equal the stdout of the command's host route for that file, with the host text of the
state-2 pairs cut from that stdout by the pair table -- as one run, and in pieces of 1 000 compressed bytes (several runs, a window each)."""
import struct
import zlib

import pytest

import signal_device_cases as sc
import signal_window_cases as wc
from pansvr_amd import signal_step as ss
from pansvr_amd.sort import BamStore

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker():
    return sc.build("signal_device_check", sc.tmpdir("swg"), False)


def members_of(recs, inflated=600):
    """the BAM file of these records as BGZF members of at most `inflated` bytes of records each, the header in front of the first one's:
    ([member], the header's inflated bytes)"""
    text = "@HD\tVN:1.6\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in sc.REFS)
    h = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(sc.REFS))
    for n, l in sc.REFS:
        h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    body = b"".join(recs)
    out = []
    if not body:                                                         # (no member holds a record: nothing to append, a run over an empty store)
        return [b""], len(h)
    for chunk in [h + body[:inflated]] + [body[o:o + inflated] for o in range(inflated, len(body), inflated)]:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return out, len(h)


def pieces_of(members, piece):
    """whole members side by side, as many as fit `piece` bytes (at least one); None: all in one"""
    if piece is None:
        return [b"".join(members)]
    out = [members[0]]                                                   # (the header's member first, with its skip)
    for m in members[1:]:
        if len(out) > 1 and len(out[-1]) + len(m) <= piece:
            out[-1] += m
        else:
            out.append(m)
    return out


def windows(recs, s, pairs, piece):
    """the windows' text over all runs, the runs, the last window's info; every run's states are held to the expected pairs on the way"""
    members, header = members_of(recs)
    st, sig = BamStore(), ss.Signal(sc.opt_of(s, []))
    got, at, runs, w = b"", 0, 0, None
    try:
        for k, p in enumerate(pieces_of(members, piece)):
            assert not p or st.append_bgzf(p, skip=header if k == 0 else 0, n_ref=len(sc.REFS)) == len(p)
            info = sig.run(st)
            runs += 1
            n_front = info.first_error if info.first_error >= 0 else info.pairs
            mine = pairs[at:at + n_front]
            assert sig.pairs()["state"][:n_front].tolist() == [x for x, _ in mine]
            host = [t for x, t in mine if x == 2]
            off = [0]
            for t in host:
                off.append(off[-1] + len(t))
            w = sig.window(b"".join(host), off)
            assert (w.n_bytes, w.n_pairs, w.n_host_pairs) == (info.text_bytes + off[-1], info.written + info.declined, len(host)) and info.declined == len(host)
            text = sig.window_text()
            assert text == b"".join(t for _, t in mine)
            got += text
            at += n_front
            if info.first_error >= 0:
                break
            st.drop(info.consumed)
        assert at == len(pairs)
        return got, runs, w
    finally:
        sig.close(), st.close()


@pytest.fixture(scope="module")
def cases(checker):
    """name: (records, summary, [(state, text)], text)"""
    out = {}
    for name, (states, error) in wc.PATTERNS.items():
        recs, front = wc.records(states, error=error)
        s, tab, text = wc.expected(recs, front, sc.tmpdir("swg"), checker)
        out[name] = (recs, s, wc.cut_by_table(text, tab), text)
    return out


@pytest.mark.parametrize("piece", [None, 1000])
@pytest.mark.parametrize("name", sorted(wc.PATTERNS))
def test_window_text_equals_the_host_routes_stdout(cases, name, piece):
    recs, s, pairs, text = cases[name]
    got, runs, _ = windows(recs, s, pairs, piece)
    assert got == text
    if piece and len(b"".join(recs)) > 5000:
        assert runs > 4


def test_window_lengths_around_a_tile_and_ranges_of_the_text(checker):
    tmp = sc.tmpdir("swg")
    have = len(wc.host_route(wc.sized_records(0), tmp, wc.ISIZE)[0])
    whole = (have // wc.TILE + 1) * wc.TILE
    for target in (whole, whole + 1):
        recs = wc.sized_records(target - have)
        s, tab, text = wc.expected(recs, recs, tmp, checker)
        assert len(text) == target == 2 * wc.TILE + (target - whole)
        got, runs, w = windows(recs, s, wc.cut_by_table(text, tab), None)
        assert got == text and runs == 1 and w.n_bytes == target


def test_ranges_refusals_and_the_windows_life(cases):
    recs, s, pairs, text = cases["alternating"]
    members, header = members_of(recs)
    st, sig = BamStore(), ss.Signal(sc.opt_of(s, []))
    try:
        st.append_bgzf(b"".join(members), skip=header, n_ref=len(sc.REFS))
        with pytest.raises(ss.EngineError, match="no run"):
            sig.window()
        info = sig.run(st)
        with pytest.raises(ss.EngineError, match="no window"):
            sig.window_text(0, 0)
        host = [t for x, t in pairs if x == 2]
        off = [0]
        for t in host:
            off.append(off[-1] + len(t))
        blob = b"".join(host)
        for why, args in (("not the number", (blob[:off[-2]], off[:-1])), ("not the number", (blob, off + [off[-1]])), ("not monotone", (blob, off[:2] + [off[1] - 1] + off[3:])),
                          ("last offset", (blob + b"x", off)), ("first offset", (blob, [1] + off[1:]))):
            with pytest.raises(ss.EngineError, match="psvr error 1: .*" + why):
                sig.window(*args)
        w = sig.window(blob, off)
        assert w.n_bytes == len(text) and sig.window_text() == text
        for first, n in ((0, 0), (0, 1), (1, 15), (15, 4097), (len(text) - 1, 1), (len(text), 0), (16384, 16)):
            assert sig.window_text(first, n) == text[first:first + n]
        for first, n in ((-1, 1), (0, len(text) + 1), (len(text), 1), (len(text) + 1, 0)):
            with pytest.raises(ss.EngineError, match="psvr error 1"):
                sig.window_text(first, n)
        assert sig.window(blob, off).n_bytes == len(text) and sig.window_text() == text      # a second window of the same run
        sig.run(st)                                                      # the next run: the window is gone
        with pytest.raises(ss.EngineError, match="no window"):
            sig.window_text(0, 1)
        assert info.declined == len(host)
    finally:
        sig.close(), st.close()
