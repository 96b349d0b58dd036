"""The layout arithmetic of the device pool's guard mode (csrc/pcv_pool_guard.h) under the host sanitizers: where the user
pointer and the two fences of a request stand in a block, and what the scan of the fences reports. The expected figures are
worked out here from the contract (256 bytes in front, the back fence from the requested byte count to the block's end and at
least 256 bytes past the rounded request), not read off the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (requested, block_bytes or 0 for the exact block, fill). 100 003 in a block of 114 944: the cache's loose match may hand a
# request a block up to bytes / 8 + 64 KiB larger than it asked for.
CASES = [(0, 0, 0), (1, 0, 0), (255, 0, 1), (256, 0, 0x4B), (257, 0, 0), (257, 4096, 0x4B), (100_003, 114_944, 0), (1, 66_048, 0xC5),
         (256, 512, 0)]


def rounded(requested):
    return (requested + 255) // 256 * 256


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pool_guard")
    (tmp / "cases.txt").write_text("".join("%d %d %d\n" % c for c in CASES))
    exe = tmp / "pool_guard_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing to preload
                           os.path.join(ROOT, "tests", "pool_guard_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp / "cases.txt")], capture_output=True, text=True)
    cases, key = {}, None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "case":
            key = (int(f[1]), int(f[2]), int(f[3]))
            cases[key] = {"damage": {}}
        elif f[0] == "damage":
            cases[key]["damage"][f[1]] = (int(f[2]), None if f[3] == "none" else int(f[3]))
        else:
            cases[key][f[0]] = f[1:]
    return p, cases


def test_sanitizer_build_of_the_guard_layout_runs_clean(driver_output):
    p, cases = driver_output
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr)[-3000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    assert len(cases) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-in-%d-fill%02x" % c)
def test_layout_and_scan(driver_output, case):
    _, cases = driver_output
    requested, block, fill = case
    exact = 256 + rounded(requested) + 256
    if block == 0:
        block = exact
    got = cases[(requested, block, fill)]
    if block < exact:
        assert got["layout"] == ["too-small"]
        return
    block_bytes, user_off, back_off, back_bytes, canary = map(int, got["layout"])
    assert block_bytes == block and user_off == 256 and user_off % 256 == 0
    assert back_off == 256 + requested, "the back fence begins at the requested byte, not at the rounded one"
    assert back_off + back_bytes == block and back_bytes >= 256 + rounded(requested) - requested
    assert canary != fill and 0 <= canary <= 255
    assert got["painted"] == ["-1"]
    d = got["damage"]
    assert d["none"][1] is None
    assert d["front_first"] == (-256, -256) and d["front_last"] == (-1, -1)
    assert d["back_first"] == (requested, requested)
    assert d["back_last"] == (block - 256 - 1, block - 256 - 1)
    assert d["both"][1] == -1
    assert d["own_last"][1] is None
