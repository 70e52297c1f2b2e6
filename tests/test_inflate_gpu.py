"""psvr_bgzf_decompress on the device (k_bgzf_inflate: a wavefront per member, pansvr_amd/csrc/inflate_device.h) against zlib: the valid
members of tests/test_inflate.py, one batch of 256 MB, and the malformed sets -- PSVR_ERR_IO naming the right member and the status the host
build of the decoder gives it (for the members made by hand: the status of the rule they break), the process alive, the members in front
of the bad one intact, and in one batch of refused and good members in turn every good member's bytes."""
import struct
import tempfile

import numpy as np
import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu


def through_device(members, datas):
    from pansvr_amd import bgzf
    out, offs, used = bgzf.bgzf_decompress(b"".join(members))
    assert used == sum(len(m) for m in members)
    assert len(offs) == len(members) + 1 and list(offs) == list(np.cumsum([0] + [len(d) for d in datas]))
    want = b"".join(datas)
    assert len(out) == len(want)
    if out.tobytes() != want:
        bad = [k for k in range(len(members)) if out[offs[k]:offs[k + 1]].tobytes() != datas[k]]
        raise AssertionError("members %s differ" % bad[:10])


def test_valid_members_through_the_abi():
    from pansvr_amd import bgzf
    golden = ic.golden_members()
    gold_data = [ic.oracle(m) for m in golden]
    assert len(golden) == 362
    through_device(golden, gold_data)
    cases = ic.zlib_members() + ic.hand_valid()
    through_device([c[1] for c in cases], [c[2] for c in cases])          # a smaller batch on the same context
    own, data = ic.own_encoder_members(tempfile.mkdtemp(prefix="psvr_inflate_"))
    through_device(own, [data[i * 16384:(i + 1) * 16384] for i in range(len(own))])
    through_device(golden + [c[1] for c in cases] + golden, gold_data + [c[2] for c in cases] + gold_data)      # and a larger one
    through_device(golden[:1], gold_data[:1])
    # a buffer that ends inside a member: the whole members in front of it are consumed
    buf = b"".join(golden[:5])
    for cut in (1, 17, 18, 30, len(golden[5]) - 1):
        out, offs, used = bgzf.bgzf_decompress(buf + golden[5][:cut])
        assert used == len(buf) and len(offs) == 6 and out.tobytes() == b"".join(gold_data[:5])
    assert bgzf.bgzf_sizes(buf + golden[5][:40]) == (len(buf), sum(len(d) for d in gold_data[:5]), 5)
    out, offs, used = bgzf.bgzf_decompress(b"")
    assert used == 0 and len(out) == 0 and list(offs) == [0]


def test_a_batch_of_256_mb():
    from pansvr_amd import bgzf
    data = ic.bam_like_big(256 << 20, 31)
    members = ic.members_of(data)
    assert len(members) == ((256 << 20) + 0xff00 - 1) // 0xff00        # several times more wavefronts than the chip holds at once
    out, offs, used = bgzf.bgzf_decompress(b"".join(members))
    assert used == sum(len(m) for m in members) and len(out) == len(data)
    got = out.tobytes()
    if got != data:
        bad = [k for k in range(len(members)) if got[k * 0xff00:(k + 1) * 0xff00] != data[k * 0xff00:(k + 1) * 0xff00]]
        raise AssertionError("%d members differ, first %s" % (len(bad), bad[:10]))


def test_malformed_members_are_an_answer():
    """First the sanitizer build of the decoder's host form on the same cases: if that is not clean, nothing is sent to the device."""
    from pansvr_amd import bgzf
    golden = ic.golden_members()
    sets = ic.malformed_sets(golden)
    assert len(sets["payload mutations"]) == 2000 and len(sets["header mutations"]) == 500
    checker = ic.build_checker(tempfile.mkdtemp(prefix="psvr_inflate_"), True)
    K = ic.constants(checker)
    named = {"by hand": ic.hand_bad(), "rule edges": ic.rule_edges()}           # the sets whose members name the status they must get
    host = {}
    for name, bufs in sets.items():
        got = ic.run_checker(checker, bufs)
        host[name] = [status for status, _ in got]
        for k, (buf, (status, out)) in enumerate(zip(bufs, got)):
            want = ic.oracle(buf)
            assert (status == 0) == (want is not None) and out == want, "host build, %s, case %d" % (name, k)
        if name in named:
            assert [c[1] for c in named[name]] == bufs
            for c, status in zip(named[name], host[name]):
                assert status == K[c[2]], "host build, %s: status %d, not %s" % (c[0], status, c[2])
    front = [m for m in golden if 200 < len(m) < 3000][:2]
    assert len(front) == 2
    front_data = b"".join(ic.oracle(m) for m in front)
    head = b"".join(front)
    seen = {"ok": 0, "bad": 0, "cut": 0}
    statuses = {}
    for name, bufs in sets.items():
        for k, buf in enumerate(bufs):
            kind = ic.classify(buf)
            seen[kind] += 1
            what = "%s, case %d (%s)" % (name, k, kind)
            try:
                out, offs, used = bgzf.bgzf_decompress(head + buf)
            except bgzf.BgzfError as e:
                assert kind == "bad", what
                assert e.bad_member == 2 and "member 2 at byte %d" % len(head) in str(e), what + ": " + str(e)
                assert e.valid_bytes == front_data, what
                # the device's status is the host build's, member for member; for the members made by hand, the one the case names.  (A member
                # refused where the batch is laid out -- its header, or an ISIZE out of its payload's reach -- never reaches the decoder.)
                want = host[name][k] if ic.header_rules(buf) and ic.inf_isize_possible(buf) else K["kInfHeader"]
                assert "(status %d)" % want in str(e), what + ": " + str(e) + ", the host build says %d" % want
                if name in named and want != K["kInfHeader"]:
                    assert want == K[named[name][k][2]], what
                statuses.setdefault(name, set()).add(want)
                continue
            assert kind != "bad", what
            if kind == "cut":
                assert used == len(head) and out.tobytes() == front_data, what
            else:
                assert used == len(head) + ic.header_rules(buf)[0] and out.tobytes() == front_data + ic.oracle(buf), what
    assert min(seen.values()) > 0, seen
    rev = {v: k for k, v in K.items()}
    for name in named:
        print("%s: the device returned %s" % (name, " ".join(sorted(rev[s] for s in statuses[name]))))
        assert statuses[name] >= {K[c[2]] for c in named[name] if c[2] != "kInfOk"}, name
    through_device(golden[:20], [ic.oracle(m) for m in golden[:20]])      # the process and the context are alive


def test_one_batch_of_rule_edges_refused_members_leave_their_neighbours_alone():
    """every member of inflate_cases.rule_edges() in ONE call, a good member between any two: one launch, a wavefront per member.  The call names the
    first refused member and its status; psvr_bgzf_decompress has copied the whole batch's output back by then, and in it every good member and
    every inside-the-edge member holds its bytes, whatever the refused members next to them did with their own slices."""
    import ctypes as C
    from pansvr_amd import bgzf, lib
    cases = ic.rule_edges()
    checker = ic.build_checker(tempfile.mkdtemp(prefix="psvr_inflate_"), True)
    K = ic.constants(checker)
    host = ic.run_checker(checker, [c[1] for c in cases])                       # the sanitizer build first, on the identical bytes
    assert [s for s, _ in host] == [K[c[2]] for c in cases]
    good = [m for m in ic.golden_members() if 200 < len(m) < 3000][:3]
    good_data = [ic.oracle(m) for m in good]
    members, want = [good[0]], [good_data[0]]
    for k, c in enumerate(cases):
        members += [c[1], good[(k + 1) % 3]]
        want += [c[3], good_data[(k + 1) % 3]]
    assert 200 < len(members) < 1000
    buf = np.frombuffer(b"".join(members), dtype=np.uint8)
    rc, used, total, nm, bad = bgzf._call(0, buf, None, 0, None, 0)
    assert (rc, used, nm, bad) == (0, len(buf), len(members), -1)                # every header passes, every ISIZE is within its payload's reach
    isizes = [struct.unpack("<I", m[-4:])[0] for m in members]
    assert total == sum(isizes)
    out = np.full(total + 64, 0xa5, dtype=np.uint8)
    offs = np.zeros(nm + 1, dtype=np.int64)
    rc, used, total, nm, bad = bgzf._call(0, buf, out.ctypes.data_as(C.c_void_p), total, offs.ctypes.data_as(C.c_void_p), nm)
    first = next(k for k, w in enumerate(want) if w is None)
    assert rc == 5 and bad == first and list(offs) == list(np.cumsum([0] + isizes))
    msg = lib().psvr_last_error().decode()
    assert "member %d at byte" % first in msg and "(status %d)" % K[cases[(first - 1) // 2][2]] in msg, msg
    assert out[total:].tobytes() == b"\xa5" * 64                                 # nothing behind the batch's last slice
    for k, w in enumerate(want):
        if w is not None:
            assert out[offs[k]:offs[k + 1]].tobytes() == w, "member %d (%s)" % (k, "a good one" if k % 2 == 0 else cases[(k - 1) // 2][0])
    through_device(good, good_data)


def test_commands_with_inflate_device_write_the_same_files():
    """`panSVR signal`, `signal -N` and `aln ... in.bam` on the inputs of the golden fused runs (test_fused_signal.GOLDEN, and a
    position-sorted generated BAM for `signal`), `sort` on the four golden fused BAM files, with --inflate-device against the default route,
    at the default chunk size and at PSVR_INFLATE_BATCH=70000: every output file byte for byte."""
    import os
    import struct
    import subprocess
    import aln_common as ac
    import test_signal as ts
    from test_fused_signal import GOLDEN, bam_of
    tmp = tempfile.mkdtemp(prefix="psvr_infl_cli_")
    recs, refs = ts.make_pairs(99, 3000)

    def key(i):
        tid, pos = struct.unpack_from("<ii", recs[i], 4)
        return (tid if tid >= 0 else 1 << 31, pos, i)
    by_pos = os.path.join(tmp, "pos.bam")
    ts.write_bam(by_pos, [recs[i] for i in sorted(range(len(recs)), key=key)], refs)
    t = lambda n: os.path.join(tmp, n)                                         # noqa: E731
    jobs = [("signal", [ts.CLI, "signal", "-D"], ["-H", t("h2"), "-S", t("s2"), by_pos], ("h2", "s2"))]
    assert len(GOLDEN) == 2
    for name, rname, n_pairs, flags in GOLDEN:
        bam = t(name + ".bam")
        bam_of(name, rname, n_pairs, bam)
        jobs.append(("signal -N " + name, [ts.CLI, "signal", "-N"] + flags, ["-H", t("h1"), "-S", t("s1"), bam], ("h1", "s1")))
        jobs.append(("aln " + name, [ts.CLI, "aln", "-N"] + flags + ["-o", t("o.bam"), "-p", t("p.bam")], [ac.index_dir(name), bam, t("h.sam")], ("o.bam", "p.bam", "h.sam")))
    fused = sorted(f for f in os.listdir(os.path.join(ac.HERE, "golden", "fused")) if f.endswith(".bam"))
    assert len(fused) == 4
    for f in fused:
        jobs.append(("sort " + f, [ts.CLI, "sort", "-o", t("sorted.bam")], [os.path.join(ac.HERE, "golden", "fused", f)], ("sorted.bam", "sorted.bam.bai")))

    def run(extra, batch):
        env = dict(os.environ)
        env.pop("PSVR_INFLATE_BATCH", None)
        if batch:
            env["PSVR_INFLATE_BATCH"] = batch
        out = {}
        for name, head, tail, outs in jobs:
            for n in outs:
                if os.path.exists(t(n)):
                    os.remove(t(n))
            r = subprocess.run(head + extra + tail, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            assert r.returncode == 0, (name, extra, r.stderr.decode()[-1500:])
            if extra:
                assert "host threads" not in r.stderr.decode(), (name, r.stderr.decode()[-1500:])      # the device route was taken and kept
            out[name] = [r.stdout if name.startswith("signal") else b""] + [open(t(n), "rb").read() for n in outs]
        return out
    want = run([], None)
    assert all(len(want[n][0]) > 10000 for n in want if n.startswith("signal")) and all(len(want[n][1]) > 10000 for n in want if n.startswith("aln"))
    for batch in (None, "70000"):
        got = run(["--inflate-device"], batch)
        for name in want:
            assert got[name] == want[name], (name, batch)
