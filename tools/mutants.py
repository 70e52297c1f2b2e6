#!/usr/bin/env python3
"""One-token mutants of the headers that are compiled for host and device, run against the CPU test file that holds each header.
  python tools/mutants.py [--jobs N] [--only TEXT] [--markdown FILE]
For every entry of MUTANTS the tree is copied to a temporary directory, `old` (which must occur exactly once in the file) is replaced by `new`, and
`python -m pytest -m "not gpu" -x <test file>` is run in the copy: a failing run has killed the mutant, a passing one lets it survive.  Every test
file is first run on an unmutated copy and must pass there.  Nothing marked gpu is ever run; no GPU is needed.  Not part of the suite: a mutant
takes as long as its test file.  The table this prints is kept in profiles/mutants_decoders.md."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, CHAIN = "pansvr_amd/csrc/inflate_device.h", "pansvr_amd/csrc/bam_chain_device.h"
T_INF, T_CHAIN = "tests/test_inflate.py", "tests/test_bam_chain.py"

# (file, old text, new text, CPU test file)
MUTANTS = [
    # ---- inflate_device.h: every rule that refuses a member, relaxed by one
    (INF, "nl > 286 || nd > 30", "nl > 287 || nd > 31", T_INF),
    (INF, "nl > 286", "nl > 287", T_INF),
    (INF, "nd > 30", "nd > 31", T_INF),
    (INF, "s >= 286", "s >= 287", T_INF),
    (INF, "d >= 30", "d >= 31", T_INF),
    (INF, "li == 28 ? 258u", "li == 28 ? 257u", T_INF),
    (INF, "dist > w.o", "dist > w.o + 1", T_INF),
    (INF, "bsize < hdr + 8u", "bsize < hdr + 7u", T_INF),
    (INF, "hdr < 12u", "hdr < 11u", T_INF),
    (INF, "if (b.n < 3) return kInfTruncated;\n\t\tlast", "if (b.n < 2) return kInfTruncated;\n\t\tlast", T_INF),
    (INF, "type == 3", "type == 4", T_INF),
    (INF, "b.n < 32", "b.n < 31", T_INF),
    (INF, "(len ^ 0xffffu) != nlen", "(len ^ 0xffffu) > nlen", T_INF),
    (INF, "len > b.end - at", "len > b.end - at + 1", T_INF),
    (INF, "kInfTruncated;\n\t\t\tif (len > isize - w.o)", "kInfTruncated;\n\t\t\tif (len > isize - w.o + 1)", T_INF),
    (INF, "b.n < 14", "b.n < 13", T_INF),
    (INF, "b.refill();\n\t\t\t\t\tif (b.n < 3)", "b.refill();\n\t\t\t\t\tif (b.n < 2)", T_INF),
    (INF, "rc != 0) return kInfCodeLengths", "rc == 1) return kInfCodeLengths", T_INF),
    (INF, "b.n < 7 && b.pos >= b.end", "b.n < 6 && b.pos >= b.end", T_INF),
    (INF, "b.n < eb", "b.n + 1 < eb", T_INF),
    (INF, "s == 16 && i == 0", "s == 16 && i < 0", T_INF),
    (INF, "(uint32_t)i + rep > (uint32_t)(nl + nd)", "(uint32_t)i + rep > (uint32_t)(nl + nd) + 1u", T_INF),
    (INF, "INF_UNI(t->lens[256]) == 0", "INF_UNI(t->lens[256]) == 16", T_INF),
    (INF, "rc == 1 || (rc == 2 && mx != 1)) return kInfLitTable", "rc == 3 || (rc == 2 && mx != 1)) return kInfLitTable", T_INF),
    (INF, "(rc == 2 && mx != 1)", "(rc == 2 && mx > 2)", T_INF),
    (INF, "rc == 1 || (rc == 2 && mx > 1)) return kInfDistTable", "rc == 3 || (rc == 2 && mx > 1)) return kInfDistTable", T_INF),
    (INF, "rc == 2 && mx > 1", "rc == 2 && mx > 2", T_INF),
    (INF, "s)) return b.n < 15 && b.pos >= b.end ? kInfTruncated : kInfLitCode", "s)) return b.n < 14 && b.pos >= b.end ? kInfTruncated : kInfLitCode", T_INF),
    (INF, "d)) return b.n < 15 && b.pos >= b.end ? kInfTruncated : kInfDistCode", "d)) return b.n < 14 && b.pos >= b.end ? kInfTruncated : kInfDistCode", T_INF),
    (INF, "w.o >= isize", "w.o > isize", T_INF),
    (INF, "b.n < leb", "b.n + 1 < leb", T_INF),
    (INF, "b.n < deb", "b.n + 1 < deb", T_INF),
    (INF, "kInfFarBack;\n\t\t\tif (len > isize - w.o)", "kInfFarBack;\n\t\t\tif (len > isize - w.o + 1)", T_INF),
    (INF, "if (l > b.n) return false", "if (l > b.n + 1) return false", T_INF),
    (INF, "w.o != isize", "w.o + 1 < isize", T_INF),
    (INF, "want_n != isize", "want_n > isize", T_INF),
    (INF, "crc == want_crc ? kInfOk", "crc != want_crc ? kInfOk", T_INF),
    # ---- bam_chain_device.h: chain_record's comparisons and the settle step's link test
    (CHAIN, "bs < kBamRecMinBlock", "bs <= kBamRecMinBlock", T_CHAIN),
    (CHAIN, "bs > kBamRecStoreMaxBlock", "bs >= kBamRecStoreMaxBlock", T_CHAIN),
    (CHAIN, "if (end - at < 4) return kChainCutHead", "if (end - at < 3) return kChainCutHead", T_CHAIN),
    (CHAIN, "end - at < kBamRecHead", "end - at < kBamRecHead - 1", T_CHAIN),
    (CHAIN, "*len > end - at", "*len > end - at + 1", T_CHAIN),
    (CHAIN, "g.guess == mine", "g.guess <= mine", T_CHAIN),
    (CHAIN, "g.guess == mine", "g.guess >= mine", T_CHAIN),
    # ---- the encoders, the emitter, the parser and the name keys
    ("pansvr_amd/csrc/deflate_wave_device.h", "d > 32768u", "d > 32767u", "tests/test_deflate_wave.py"),
    ("pansvr_amd/csrc/deflate_wave_device.h", "n - p : 258u", "n - p : 257u", "tests/test_deflate_wave.py"),
    ("pansvr_amd/csrc/deflate_wave_device.h", "l > best", "l >= best", "tests/test_deflate_wave.py"),
    ("pansvr_amd/csrc/bam_emit_device.h", "x >= -32768", "x >= -32769", "tests/test_bam_emit_device.py"),
    ("pansvr_amd/csrc/bam_emit_device.h", "x <= 65535", "x <= 65536", "tests/test_bam_emit_device.py"),
    ("pansvr_amd/csrc/fastq_device.h", "sp > 65535u ? 65535u", "sp > 65535u ? 65534u", "tests/test_fastq_parse.py"),
    ("pansvr_amd/csrc/name_key.h", "nbytes >= 8", "nbytes >= 7", "tests/test_name_key.py"),
]

SKIP = shutil.ignore_patterns(".git", "build", "_ref", "__pycache__", "*.o", "*.pyc", ".pytest_cache", "profiles", "parent_bin")


def run_tests(tree, test):
    t0 = time.time()
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "not gpu", "-x", "-q", "-p", "no:cacheprovider", test], cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    tail = [l for l in r.stdout.decode(errors="replace").split("\n") if l.startswith(("FAILED", "ERROR"))]
    return r.returncode, time.time() - t0, (tail[0].split(" - ")[0] if tail else "")


def one(entry, base):
    """the verdict on one mutant: its own copy of `base` (an unmutated copy of the tree), the edit, the test file"""
    path, old, new, test = entry
    tree = tempfile.mkdtemp(prefix="psvr_mutant_")
    try:
        shutil.copytree(base, os.path.join(tree, "t"), symlinks=True)
        fn = os.path.join(tree, "t", path)
        text = open(fn).read()
        if text.count(old) != 1:
            return "the old text occurs %d times" % text.count(old), 0.0, ""
        with open(fn, "w") as f:
            f.write(text.replace(old, new))
        rc, secs, first = run_tests(os.path.join(tree, "t"), test)
        return ("killed" if rc else "survived"), secs, first
    finally:
        shutil.rmtree(tree, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--only", default="", help="only the mutants whose file, old text or test file contains this")
    ap.add_argument("--markdown", default="", help="write the table to this file as well")
    a = ap.parse_args()
    todo = [m for m in MUTANTS if a.only in m[0] or a.only in m[1] or a.only in m[3]]
    base = tempfile.mkdtemp(prefix="psvr_mutants_base_")
    failed = False
    try:
        shutil.copytree(ROOT, os.path.join(base, "t"), ignore=SKIP, symlinks=True)
        tree = os.path.join(base, "t")
        for test in sorted({m[3] for m in todo}):
            rc, secs, first = run_tests(tree, test)
            print("unmutated %s: %s in %.0f s" % (test, "passes" if rc == 0 else "FAILS (%s)" % first, secs), flush=True)
            failed |= rc != 0
        if failed:
            return 2
        with ThreadPoolExecutor(a.jobs) as ex:
            results = list(ex.map(lambda m: one(m, tree), todo))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    rows = ["| file | mutant | test file | result | first failing test |", "|---|---|---|---|---|"]
    for (path, old, new, test), (verdict, secs, first) in zip(todo, results):
        show = lambda s: " ".join(s.split()).replace("|", "\\|")                # noqa: E731
        rows.append("| `%s` | `%s` -> `%s` | `%s` | %s | %s |" % (os.path.basename(path), show(old), show(new), os.path.basename(test), verdict if verdict != "survived" else "**survived**",
                                                               first.replace("FAILED ", "").split("::")[-1] if first else ""))
        failed |= verdict not in ("killed", "survived")
    table = "\n".join(rows)
    print(table)
    n_s = sum(r[0] == "survived" for r in results)
    print("\n%d mutants: %d killed, %d survived" % (len(results), sum(r[0] == "killed" for r in results), n_s))
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(table + "\n")
    return 2 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
