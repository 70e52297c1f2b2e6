"""-m gpu: `panSVR signal --mate-device` on the MI355X against plain `panSVR signal` of the same build on the same position-sorted file: stdout
byte for byte, the header file, the status file, and stderr less the route's one line; the summary line says that pairs were written on the
device and what the store held behind the last block.  No input the host loop aborts on is run here (tests/test_signal_pos_route.py holds
those on the CPU).  Every command is a child of its own under a time limit."""
import os
import re

import pytest

import signal_mate_cases as mc

pytestmark = pytest.mark.gpu
STAT_LINE = re.compile(rb"signal --mate-device: (\d+) pairs, (\d+) written on the device, (\d+) declined to the host, (\d+) paired by name, (\d+) blocks, (\d+) text bytes, "
                       rb"peak footprint (\d+) chunks \((\d+) bytes\), (\d+) chunks \((\d+) bytes\) behind the last block")


@pytest.fixture(scope="module")
def files():
    tmp = mc.sc.tmpdir("mdg")
    recs, refs = mc.make_pairs_sorted(20241, 1500)
    mc.ts.write_bam(os.path.join(tmp, "pairs.bam"), recs, refs)
    return tmp, {"pairs": os.path.join(tmp, "pairs.bam"), "crafted": mc.write(os.path.join(tmp, "crafted.bam"), mc.crafted()),
                 "decreasing": mc.write(os.path.join(tmp, "dec.bam"), mc.decreasing())}


def both(files, name, flags, env=None):
    tmp, f = files
    h = mc.run_cmd(mc.CLI, tmp, f[name], flags, "h")
    d = mc.run_cmd(mc.CLI, tmp, f[name], flags + ["--mate-device"], "d", env=env)
    assert h[0].returncode == 0 and d[0].returncode == 0, d[0].stderr.decode()[-2000:]
    assert d[0].stdout == h[0].stdout and d[1] == h[1] and d[2] == h[2] and h[1] and h[2]
    own = mc.own_lines(d[0].stderr)
    assert len(own) == 1, d[0].stderr.decode()[-2000:]
    assert mc.without(d[0].stderr, own) == h[0].stderr
    return own[0], h[0].stdout


@pytest.mark.parametrize("name", ["pairs", "crafted"])
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
def test_device_route_writes_the_host_routes_files(files, name, flags):
    line, out = both(files, name, flags)
    m = STAT_LINE.search(line)
    assert m, line
    pairs, written, declined, by_name, blocks, text_bytes = [int(x) for x in m.groups()[:6]]
    assert blocks >= 5 and by_name > 0 and pairs > by_name and (name != "pairs" or written > 0)
    if flags == ["-D"]:
        assert written > 0 and 0 < text_bytes <= len(out) and (name != "pairs" or (pairs == 1500 and written > 500))


@pytest.mark.parametrize("piece", [1000, 70000])
@pytest.mark.parametrize("block", [64, None])
def test_pieces_and_block_sizes(files, piece, block):
    line, _ = both(files, "pairs", ["-D"] + (["--block-records", str(block)] if block else []), {"PSVR_INFLATE_BATCH": str(piece)})
    m = STAT_LINE.search(line)
    assert m and int(m.group(1)) == 1500 and int(m.group(2)) > 0, line
    line, _ = both(files, "crafted", ["-D", "-U"] + (["--block-records", str(block)] if block else []), {"PSVR_INFLATE_BATCH": str(piece)})
    assert STAT_LINE.search(line), line


def test_the_footprint_behind_the_last_block_is_bounded_by_a_block_and_a_chunk(files):
    chunk = 80000
    line, _ = both(files, "pairs", ["-D", "--block-records", "64"], {"PSVR_INFLATE_BATCH": "20000", "PSVR_BAM_STORE_CHUNK_BYTES": str(chunk), "PSVR_BAM_STORE_SEG_BYTES": "4096"})
    m = STAT_LINE.search(line)
    assert m, line
    pairs, peak_chunks, peak_bytes, last_chunks, last_bytes = int(m.group(1)), int(m.group(7)), int(m.group(8)), int(m.group(9)), int(m.group(10))
    # about 800 KB of records in ten chunks' worth, a block (64 records, about 17 KB) far smaller than a chunk.  Behind the last block no record
    # is left: the chunk being filled and the spare that store_drop keeps, nothing else.  At the peak, in front of a drop: the chunk with the
    # carried records, the chunk a piece's append began and the one it ended in, and the spare
    assert pairs == 1500 and last_chunks <= 2 and last_bytes <= 2 * chunk and peak_chunks <= 4 and peak_bytes <= 4 * chunk
    # a block per chromosome: the pieces of a block, and the left-overs among them, lie in more than one chunk
    line, _ = both(files, "pairs", ["-D"], {"PSVR_INFLATE_BATCH": "20000", "PSVR_BAM_STORE_CHUNK_BYTES": str(chunk), "PSVR_BAM_STORE_SEG_BYTES": "4096"})
    m = STAT_LINE.search(line)
    assert m and int(m.group(1)) == 1500 and int(m.group(7)) >= 2, line


def test_decreasing_positions_leave_the_route_on_one_line(files):
    tmp, f = files
    h = mc.run_cmd(mc.CLI, tmp, f["decreasing"], ["-D"], "h")
    d = mc.run_cmd(mc.CLI, tmp, f["decreasing"], ["-D", "--mate-device"], "d")
    assert d[0].returncode == h[0].returncode == 0 and d[0].stdout == h[0].stdout and d[1] == h[1] and d[2] == h[2]
    own = mc.own_lines(d[0].stderr)
    assert len(own) == 1 and b"signal run_pos failed" in own[0] and b"positions decrease inside a block" in own[0] and b"0 pairs are written" in own[0]
