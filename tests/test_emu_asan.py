"""EngineCore's memory under AddressSanitizer / UBSan / LeakSanitizer (CPU build of the emulator only): fx2/reads150 in batches of 97
pairs with the scratch arenas started at 1/16 re-uploads batches, grows the DP buffers and regrows every arena.  The run must end without
a sanitizer report -- no buffer of the core outlives it -- and with the reference's records."""
import os
import subprocess

import pytest

import aln_common as ac
from test_emu_aln import normalise

EMU_DIR = os.path.join(ac.HERE, "emu")
EXE = os.path.join(EMU_DIR, "emu_aln_asan")


@pytest.fixture(scope="module")
def exe():
    csrc = os.path.join(ac.ROOT, "pansvr_amd", "csrc")
    src = os.path.join(EMU_DIR, "emu_main.cpp")
    deps = [src, os.path.join(ac.ROOT, "oracle", "ksw_oracle.c")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPSVR_EMU_SPARSE_HASH",
                               "-DPSVR_NO_ENGINE_LIB", "-o", EXE, src, os.path.join(ac.ROOT, "oracle", "ksw_oracle.c"), "-lz", "-lpthread"])
    return EXE


def test_engine_core_batches_and_regrowth_leak_nothing(exe):
    w = ac.workdir("fx2")
    env = dict(os.environ, PSVR_ARENA_SHRINK="16", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe, os.path.join(ac.golden_dir("fx2"), "idx"), os.path.join(w, "reads150.fq"), os.path.join(w, "header.sam"), "--trace", "--batch", "97"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert r.returncode == 0, (r.returncode, err[-1000:])
    assert "scratch arena overflow" in err
    got = [l for l in r.stdout.decode().split("\n") if l.strip()]
    want = ac.golden_lines("fx2", "reads150")
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(want, got)) if normalise(a) != normalise(b)]
    assert not bad, "%d/%d pairs differ; first %d" % (len(bad), len(want), bad[0])
