"""-m gpu: psvr_fastq_parse_signal on the MI355X against psvr_fastq_parse of the same bytes from the host: every downloaded array, the info and
psvr_fastq_text -- with max_pairs of 1, 37 and unlimited, a window walked to its end by used_bytes, a max_bases cut, a window of 0 bytes and
first_byte == n_bytes."""
import numpy as np
import pytest

import signal_device_cases as sc
import signal_window_cases as wc
from pansvr_amd import signal_step as ss
from pansvr_amd.fastq import FastqParser
from pansvr_amd.sort import BamStore
from test_signal_window_gpu import members_of

pytestmark = pytest.mark.gpu

UNLIMITED = 1 << 40
FIELDS = ("n_pairs", "used_bytes", "total_bases", "n_lines", "stop", "reserved")


class Window:
    """a signal object that holds the window of one pattern, its text, and the two parsers"""

    def __init__(self, name, checker):
        states, error = wc.PATTERNS[name]
        recs, front = wc.records(states, error=error)
        s, tab, self.text = wc.expected(recs, front, sc.tmpdir("fps"), checker)
        pairs = wc.cut_by_table(self.text, tab)
        members, header = members_of(recs)
        self.st, self.sig = BamStore(), ss.Signal(sc.opt_of(s, []))
        if members != [b""]:
            self.st.append_bgzf(b"".join(members), skip=header, n_ref=len(sc.REFS))
        self.sig.run(self.st)
        host = [t for x, t in pairs if x == 2]
        self.n_pairs = sum(x in (1, 2) for x, _ in pairs)
        assert self.sig.window(b"".join(host), np.concatenate([[0], np.cumsum([len(t) for t in host])]).astype(np.int64)).n_bytes == len(self.text)
        self.dev, self.host = FastqParser(), FastqParser()

    def both(self, first_byte, max_pairs, max_bases):
        """the info both routes agree on, after every array and the text have been compared"""
        a = self.dev.parse_signal(self.sig, first_byte, max_pairs, max_bases)
        b = self.host.parse(self.text[first_byte:], max_pairs, max_bases, at_end=True)
        assert [getattr(a, f) for f in FIELDS] == [getattr(b, f) for f in FIELDS]
        da, db = self.dev.download(), self.host.download()
        assert sorted(da) == sorted(db) == ["base_off", "bases", "line_start", "name_end", "ori"]
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), k
        n = len(self.text) - first_byte
        assert self.dev.text(0, n) == self.host.text(0, n) == self.text[first_byte:]
        assert self.dev.text(0, a.used_bytes) == self.text[first_byte:first_byte + a.used_bytes]
        return a

    def close(self):
        self.dev.close(), self.host.close(), self.sig.close(), self.st.close()


@pytest.fixture(scope="module")
def checker():
    return sc.build("signal_device_check", sc.tmpdir("fps"), False)


@pytest.fixture(scope="module")
def win(checker):
    w = Window("alternating", checker)
    yield w
    w.close()


@pytest.mark.parametrize("max_pairs", [1, 37, UNLIMITED])
def test_a_window_walked_to_its_end_by_used_bytes(win, max_pairs):
    at, pairs, calls = 0, 0, 0
    while True:
        i = win.both(at, max_pairs, UNLIMITED)
        if i.n_pairs == 0:
            break
        assert i.n_pairs == min(max_pairs, win.n_pairs - pairs) and i.used_bytes > 0
        at, pairs, calls = at + i.used_bytes, pairs + i.n_pairs, calls + 1
    assert at == len(win.text) and pairs == win.n_pairs == 112 and calls == -(-win.n_pairs // max_pairs)
    assert i.stop == 2 and i.used_bytes == 0                             # first_byte == n_bytes: nothing, as the host parser says of no text


def test_a_max_bases_cut_and_ranges_of_the_text(win):
    i = win.both(0, UNLIMITED, 500)
    assert i.stop == 1 and 0 < i.n_pairs < 10 and i.total_bases >= 500
    j = win.both(i.used_bytes, 37, 2000)
    assert j.stop == 1 and 0 < j.n_pairs < 37
    n = len(win.text) - i.used_bytes
    for first, m in ((0, 0), (1, 15), (15, 4097), (n - 1, 1), (n, 0)):
        assert win.dev.text(first, m) == win.text[i.used_bytes + first:i.used_bytes + first + m]
    for first, m in ((-1, 1), (0, n + 1), (n, 1), (n + 1, 0)):
        with pytest.raises(ss.EngineError, match="psvr error 1"):
            win.dev.text(first, m)


def test_refusals(win):
    for first in (-1, len(win.text) + 1):
        with pytest.raises(ss.EngineError, match="psvr error 1: .*first byte"):
            win.dev.parse_signal(win.sig, first, 1, 1)
    sig = ss.Signal(ss.signal_opt([100, 1, 2, 3], 1, 500))
    try:
        with pytest.raises(ss.EngineError, match="psvr error 1: .*no window"):
            win.dev.parse_signal(sig, 0, 1, 1)
    finally:
        sig.close()
    fq = FastqParser()
    try:
        with pytest.raises(ss.EngineError, match="psvr error 1: .*no parsed window"):
            fq.text(0, 0)
    finally:
        fq.close()


def test_a_window_of_no_bytes(checker):
    w = Window("empty_run", checker)
    try:
        assert w.text == b""
        i = w.both(0, UNLIMITED, UNLIMITED)
        assert i.n_pairs == 0 and i.used_bytes == 0 and i.stop == 2
    finally:
        w.close()


def test_the_signal_object_may_run_again_once_the_parse_has_returned(win):
    """the parser keeps the bytes: a new run (and a drop of the store) behind the call changes nothing in what it hands out"""
    i = win.dev.parse_signal(win.sig, 0, UNLIMITED, UNLIMITED)
    before = win.dev.download()
    win.sig.run(win.st)
    win.st.drop(win.st.info().n_records)
    after = win.dev.download()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before) and win.dev.text(0, i.used_bytes) == win.text
