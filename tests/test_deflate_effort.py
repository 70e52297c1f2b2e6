"""The wavefront-per-member BGZF encoder's efforts (dfw_member_effort of pansvr_amd/csrc/deflate_wave_device.h: hash chains of 4, 8, 16
and lazy matching at efforts 1, 2, 3; effort 0 is the encoder as it was) in the host build with one lane, whose bytes are the device's
(tests/test_deflate_effort_gpu.py compares them).  zlib inflates every member to its input; the plain and the sanitizer build agree;
what the token and link scratch held before does not show; a member depends on its own bytes only; effort 0 is deflate_wave_check's
encoder byte for byte.  Then the rule's edges on crafted inputs, by the tokens; the sizes on golden records against zlib; the option."""
import os
import subprocess
import tempfile

import pytest

import deflate_effort_cases as de
import deflate_wave_cases as dc
import inflate_cases as ic
import test_signal as ts

CLI = ts.CLI
BIG = 0xff00


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_dfe_")
    return de.build_checker(tmp, False), de.build_checker(tmp, True), dc.build_checker(tmp, False)


@pytest.fixture(scope="module")
def records():
    return dc.fx2_records()


@pytest.fixture(scope="module")
def crafted():
    return de.crafted()


@pytest.mark.parametrize("member_bytes", dc.MEMBER_SIZES)
@pytest.mark.parametrize("effort", de.EFFORTS)
def test_every_member_inflates_to_its_input(checkers, records, crafted, effort, member_bytes):
    plain, asan, wave = checkers
    for name, data in dc.cases(member_bytes, records) + crafted:
        raw = de.host_members(plain, data, member_bytes, effort)
        dc.check_members(raw, data, member_bytes)
        assert de.host_members(asan, data, member_bytes, effort) == raw, name                  # the sanitizer build: clean, and the same bytes
        assert de.host_members(plain, data, member_bytes, effort, dirty=True) == raw, name     # 0xff in tok and link beforehand: the same bytes
        if effort == 0:
            assert dc.host_members(wave, data, member_bytes) == raw, name                      # the encoder as it was


@pytest.mark.parametrize("effort", de.EFFORTS)
def test_a_member_depends_on_its_own_bytes_only(checkers, records, effort):
    plain = checkers[0]
    for mb in (4096, BIG):
        piece = records[:mb]
        alone = de.host_members(plain, piece, mb, effort)
        longer = ic.bam_like(2 * mb, 4) + piece + ic.bam_like(mb // 2, 6)                       # as the third member of a longer buffer
        ms = ic.split_members(de.host_members(plain, longer, mb, effort))
        assert len(ms) == 4 and ms[2] == alone
        ms = ic.split_members(de.host_members(plain, longer, mb, effort, dirty=True))
        assert len(ms) == 4 and ms[2] == alone


def _tokens(plain, data, effort):
    raw, toks = de.host_members(plain, data, BIG, effort, tokens=True)
    assert len(data) <= BIG
    return raw, toks, de.token_map(toks)


@pytest.mark.parametrize("visits", (3, 6, 10, 20))
def test_chain_reaches_the_oldest_visit_exactly_when_it_is_deep_enough(checkers, visits):
    plain = checkers[0]
    data, probes = de.chain_visits(visits, 70, 40, 6, 100 + visits)
    got = {e: _tokens(plain, data, e) for e in de.EFFORTS}
    for e in de.EFFORTS:
        reached = de.DEPTH[e] >= visits
        for at, first in probes:
            tm = got[e][2]
            if reached:
                assert tm[at] == (43, at - first), (e, at, tm[at])                             # the oldest visit's 3 + 40 bytes
            elif e == 0:
                assert tm[at] == (3, 70), (e, at, tm[at])                                      # the nearest visit's three
            else:                                                                              # ... which give way to the 2 + 40 the next position's own bucket has
                assert tm[at] == data[at] and tm[at + 1] == (42, at - first), (e, at, tm[at], tm.get(at + 1))
    sizes = {e: len(got[e][0]) for e in (1, 2, 3)}
    print("visits %d: sizes %s" % (visits, sizes))
    for a in (1, 2, 3):
        for b in (1, 2, 3):
            if (de.DEPTH[a] >= visits) == (de.DEPTH[b] >= visits):
                assert got[a][1] == got[b][1] and sizes[a] == sizes[b], (a, b)                 # the same tokens where the depth makes no difference ...
            elif de.DEPTH[a] >= visits:
                assert sizes[a] < sizes[b], (a, b, sizes)                                      # ... and a smaller member exactly where it reaches


@pytest.mark.parametrize("visits", (6, 7))
def test_no_link_and_no_match_inside_one_group(checkers, visits):
    """Visits 8 bytes apart with the probe behind them fit one group of 64 up to 7 times (the probe's last byte is the group's 64th); 10 and 20
    visits at that spacing cannot lie in one group.  Seven prior visits would separate depth 4 from depth 8 if the group linked at all."""
    plain = checkers[0]
    data, probes = de.chain_visits(visits, 8, 4, 1, 17)
    (at, first), = probes
    assert first // 64 == (at + 7) // 64                                                       # every visit and the probe's seven bytes in one group of 64
    raws = set()
    for e in de.EFFORTS:
        raw, toks, tm = _tokens(plain, data, e)
        assert not any(x & 0x80000000 for x in toks), e                                        # positions of one group do not see one another
        raws.add(raw)
    assert len(raws) == 1


def test_chain_candidate_at_distance_32768_and_beyond(checkers):
    plain = checkers[0]
    sizes = {}
    for dist in (32768, 32769):
        data, at = de.chain_far(dist)
        for e in de.EFFORTS:
            raw, toks, tm = _tokens(plain, data, e)
            sizes[dist, e] = len(raw)
            if e and dist == 32768:
                assert tm[at] == (203, 32768), (e, tm.get(at))                                 # a link behind the table's entry, at the window's edge: taken
            else:
                assert tm[at] == data[at], (dist, e, tm.get(at))                               # the walk stops (effort 0: never walks); three bytes 32468 back are too far
            assert all(v[1] <= 32768 for v in tm.values() if isinstance(v, tuple))
    for e in (1, 2, 3):
        assert sizes[32768, e] < sizes[32769, e] - 100, sizes


def test_lazy_stops_at_a_groups_last_position(checkers):
    plain = checkers[0]
    for last in (True, False):
        data, p = de.lazy_at(64 * 3 + (63 if last else 62))
        for e in de.EFFORTS:
            tm = _tokens(plain, data, e)[2]
            if e == 0 or last:
                assert tm[p][0] == 4 and p + 1 not in tm, (last, e, tm.get(p))                 # no look-ahead over the group's end: the shorter match stands
            else:
                assert tm[p] == data[p] and tm[p + 1][0] == 15, (last, e, tm.get(p), tm.get(p + 1))


def test_lazy_behind_a_match_carried_over_a_groups_end(checkers):
    plain = checkers[0]
    data, q = de.carried_then_lazy(64 * 3 + 60)
    for e in de.EFFORTS:
        tm = _tokens(plain, data, e)[2]
        assert tm[q][0] == 10 and not any(q < k < q + 10 for k in tm), (e, tm.get(q))          # covers six positions of the next group
        if e == 0:
            assert tm[q + 10][0] == 4
        else:
            assert tm[q + 10] == data[q + 10] and tm[q + 11][0] == 15, (e, tm.get(q + 10), tm.get(q + 11))


def test_distances_1_and_2_still_win_over_the_chain(checkers, records):
    plain = checkers[0]
    cs = dict(dc.cases(BIG, records))
    for name, d in (("zeros", 1), ("period 2", 2)):
        data = cs[name][:BIG]
        for e in de.EFFORTS:
            raw, toks, tm = _tokens(plain, data, e)
            ms = [v for v in tm.values() if isinstance(v, tuple)]
            assert ms and all(v[1] == d for v in ms), (name, e)
            assert len(raw) < 400, (name, e, len(raw))


def test_sizes_on_golden_records_against_zlib(checkers):
    """The size guard: the records of two golden BAMs, as they lie and reordered by (tid, pos), in members of 0xff00 bytes.  Measured with the
    rule as built (relative to zlib level 6; effort 0 1.130 1.107 1.101 1.074, effort 1 1.031 1.023 1.027 1.014, effort 2 1.017 1.011 1.017
    1.009, effort 3 1.010 1.004 1.013 1.005; zlib level 1 1.083 1.132 1.070 1.095; effort 1 / effort 0 0.913 0.924 0.933 0.945)."""
    plain = checkers[0]
    for name, data in de.size_inputs():
        z1, z6 = de.zlib_total(data, 1), de.zlib_total(data, 6)
        e = [len(de.host_members(plain, data, BIG, k)) for k in de.EFFORTS]
        print("%s: %d bytes; against zlib level 6: zlib level 1 %.3f, efforts 0..3 %s; effort 1 / effort 0 %.3f" % (name, len(data), z1 / z6, " ".join("%.3f" % (x / z6) for x in e), e[1] / e[0]))
        assert e[1] <= 0.96 * e[0], (name, e)
        assert e[1] >= e[2] >= e[3], (name, e)
        for k in (1, 2, 3):
            assert e[k] < z1, (name, k, e[k], z1)
            assert e[k] <= 1.04 * z6, (name, k, e[k], z6)


# ---- the C boundary, without launching anything ------------------------------------------------------------------------------------------------
def test_abi_refuses_an_effort_outside_0_to_3():
    import ctypes as C
    import numpy as np
    from pansvr_amd import lib
    L = lib()
    data, out = np.arange(1000, dtype=np.uint8), np.zeros(2000, dtype=np.uint8)
    total = C.c_int64(-7)
    for effort in (4, -1, 1 << 20):
        rc = L.psvr_bgzf_compress_members_effort(C.c_int(0), data.ctypes.data_as(C.c_void_p), C.c_int64(1000), C.c_int32(0), out.ctypes.data_as(C.c_void_p), C.c_int64(2000),
                                                 C.byref(total), None, C.c_int64(0), None, C.c_int32(effort))
        assert rc == 1 and b"effort" in L.psvr_last_error(), effort
    for effort in (0, 3):                                                      # no bytes: no members at any effort, and no device needed
        rc = L.psvr_bgzf_compress_members_effort(C.c_int(0), None, C.c_int64(0), C.c_int32(0), None, C.c_int64(0), C.byref(total), None, C.c_int64(0), None, C.c_int32(effort))
        assert rc == 0 and total.value == 0
    assert L.psvr_bgzf_stream_set_effort(None, C.c_int32(2)) == 1


# ---- the commands --------------------------------------------------------------------------------------------------------------------------------
def _refused(cmd, tmp_path, text):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    err = r.stderr.decode()
    assert r.returncode == 1, err
    assert text in err and len(err.strip().split("\n")) == 1, err
    assert "loading index" not in err and not os.listdir(str(tmp_path)), err


def test_deflate_effort_wants_a_route_that_uses_the_encoder(tmp_path):
    missing = [str(tmp_path / "no_idx"), str(tmp_path / "no_reads.fq"), str(tmp_path / "no_header.sam")]
    out = ["-o", str(tmp_path / "o.bam"), "-p", str(tmp_path / "p.bam")]
    for flags in ([], ["--sort"], ["--emit-device"], ["--bgzf-device"]):
        _refused([CLI, "aln", "--deflate-effort", "2"] + flags + out + missing, tmp_path, "--deflate-effort cannot be given without")
    for flags in ([], ["-n"], ["--inflate-threads", "2"]):
        _refused([CLI, "sort", "--deflate-effort", "2"] + flags + ["-o", str(tmp_path / "s.bam"), str(tmp_path / "no_in.bam")], tmp_path, "--deflate-effort cannot be given without")


@pytest.mark.parametrize("n", ("4", "-1", "x", "2x", "", "10"))
def test_deflate_effort_outside_0_to_3_is_refused(tmp_path, n):
    missing = [str(tmp_path / "no_idx"), str(tmp_path / "no_reads.fq"), str(tmp_path / "no_header.sam")]
    for route in ("--deflate-device", "--stream-device", "--sort-device"):
        _refused([CLI, "aln", route, "--deflate-effort", n, "-o", str(tmp_path / "o.bam"), "-p", str(tmp_path / "p.bam")] + missing, tmp_path, "--deflate-effort wants 0 .. 3")
    for route in ("--deflate-device", "--sort-device", "--nsort-device"):
        _refused([CLI, "sort", route, "--deflate-effort", n, "-o", str(tmp_path / "s.bam"), str(tmp_path / "no_in.bam")], tmp_path, "--deflate-effort wants 0 .. 3")


def test_deflate_effort_without_a_number_is_not_the_input_file(tmp_path):
    _refused([CLI, "sort", "--deflate-device", "-o", str(tmp_path / "s.bam"), str(tmp_path / "no_in.bam"), "--deflate-effort"], tmp_path, "--deflate-effort wants 0 .. 3")


def test_usage_lists_deflate_effort():
    for cmd in ("aln", "sort"):
        r = subprocess.run([CLI, cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and "--deflate-effort" in r.stderr.decode()
