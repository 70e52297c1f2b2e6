"""-m gpu: psvr_sort_order_names (pansvr_amd.sort.sort_order_names) on the MI355X against a restatement, Python's sorted() on (name, tie, index):
the names of tests/name_cases.py (chunk edges, prefixes, constant chunks, bytes above 0x7f), the wavefront and tile edges of sort.hip, many
ties and long shared prefixes, every name equal; and the statuses of bad arguments."""
import ctypes as C
import random

import numpy as np
import pytest

import name_cases as nc

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2, 63, 64, 65, 511, 513, 2047, 2048, 2049, 4 * 2048 + 7)


def _names_and_ties(case):
    return [f.split(b"\0")[0] for f, _ in case], [flag & 0xc0 for _, flag in case]


@pytest.mark.parametrize("group", sorted(nc.groups()))
def test_the_case_list(group):
    from pansvr_amd.sort import sort_order_names
    names, tie = _names_and_ties(nc.groups()[group])
    assert sort_order_names(names, tie).tolist() == nc.restated_order_names(names, tie)
    assert sort_order_names(names).tolist() == nc.restated_order_names(names)
    back = list(reversed(names))
    assert sort_order_names(back, tie).tolist() == nc.restated_order_names(back, tie)


_RANDOM = {}


def random_names(n):
    """n names of 1-40 random bytes over three letters (every one of the five chunks varies; a name is often a prefix of others and the
    short ones tie), and a tie key each -- made once"""
    if n not in _RANDOM:
        rng = random.Random(100 + n)
        names = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(1, 41))) for _ in range(n)]
        _RANDOM[n] = (names, [rng.choice((0, 0x40, 0x80, 0xc0)) for _ in range(n)])
    return _RANDOM[n]


def test_random_tails_behind_shared_prefixes():
    """names of 1-16 letters behind nothing or a prefix of 16 or 24 bytes: whole constant chunks in front of chunks that vary"""
    from pansvr_amd.sort import sort_order_names
    rng = random.Random(77)
    names = [rng.choice((b"", nc.P16, nc.P24)) + bytes(rng.choice(b"abc") for _ in range(rng.randrange(1, 17))) for _ in range(2049)]
    tie = [rng.choice((0, 0x40, 0x80, 0xc0)) for _ in names]
    assert sort_order_names(names, tie).tolist() == nc.restated_order_names(names, tie)
    only24 = [nc.P24 + x[-3:] for x in names]
    assert sort_order_names(only24, tie).tolist() == nc.restated_order_names(only24, tie)


@pytest.mark.parametrize("n", SIZES)
def test_wavefront_and_tile_edges_with_many_ties(n):
    from pansvr_amd.sort import sort_order_names
    names, tie = random_names(n)
    got = sort_order_names(names, tie)
    assert got.dtype == np.uint32 and got.tolist() == nc.restated_order_names(names, tie)
    assert sort_order_names(names).tolist() == nc.restated_order_names(names)
    if n >= 511:
        assert len(set(names)) < n and got.tolist() != list(range(n))          # ties there are, and an order to find


def test_short_random_names_tie_heavily():
    from pansvr_amd.sort import sort_order_names
    rng = random.Random(9)
    names = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(1, 5))) for _ in range(5000)]
    tie = [rng.randrange(256) for _ in names]                                   # the tie key is any byte
    assert sort_order_names(names, tie).tolist() == nc.restated_order_names(names, tie)


def test_equal_names_keep_the_input_order():
    from pansvr_amd.sort import sort_order_names
    names = [nc.P24 + b"same"] * 2049
    assert sort_order_names(names).tolist() == list(range(2049))                # every chunk is constant: no pass runs
    tie = [0x80 if i % 3 == 0 else 0x40 for i in range(2049)]
    assert sort_order_names(names, tie).tolist() == nc.restated_order_names(names, tie)
    assert sort_order_names([b""] * 70).tolist() == list(range(70))


def _raw(n, blob, off, tie=None):
    from pansvr_amd import lib
    b = np.frombuffer(blob, dtype=np.uint8)
    o = np.array(off, dtype=np.int64)
    t = None if tie is None else np.array(tie, dtype=np.uint8)
    out = np.full(max(len(off), 1), 0xffffffff, dtype=np.uint32)
    rc = lib().psvr_sort_order_names(C.c_int(0), C.c_int64(n), b.ctypes.data_as(C.c_void_p), C.c_int64(len(b)), o.ctypes.data_as(C.c_void_p),
                                     None if t is None else t.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_bad_arguments_and_the_library_afterwards():
    from pansvr_amd import lib
    from pansvr_amd.sort import sort_order_names
    blob = b"bb\0a\0" + b"x" * 254 + b"\0" + b"y" * 255 + b"\0" + b"tail"
    assert _raw(3, blob, [0, 3, 5])[0] == 0 and _raw(3, blob, [0, 3, 5])[1].tolist() == [1, 0, 2]      # 254 bytes are fine
    assert _raw(3, blob, [0, 3, 260])[0] == 2                                   # PSVR_ERR_UNSUPPORTED: a name of 255 bytes
    assert b"254" in lib().psvr_last_error()
    assert _raw(3, blob, [0, 3, len(blob) - 4])[0] == 1                         # PSVR_ERR_ARG: no NUL before the blob's end
    assert _raw(3, blob, [0, 3, len(blob)])[0] == 1 and _raw(3, blob, [0, -1, 3])[0] == 1    # an offset outside the blob
    assert _raw(1 << 32, blob, [0])[0] == 2                                     # the order is 32-bit
    assert _raw(-1, blob, [0])[0] == 1
    assert lib().psvr_sort_order_names(C.c_int(0), C.c_int64(2), None, C.c_int64(5), None, None, None) == 1
    assert lib().psvr_sort_order_names(C.c_int(0), C.c_int64(0), None, C.c_int64(0), None, None, None) == 0
    assert _raw(2, blob, [3, 0], [7, 7])[1][:2].tolist() == [0, 1]              # names share a blob in any order of offsets
    assert sort_order_names([b"b", b"a", b"b"], [0x80, 0, 0x40]).tolist() == [1, 2, 0]
