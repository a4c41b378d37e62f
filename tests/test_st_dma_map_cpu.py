"""The staging map of k_spmv_st_dma (macroc_amd/csrc/st_dma_map.h) checked on the host: the stand-alone
program tests/csrc/st_dma_map_check.cpp, built with AddressSanitizer + UBSan, calls the functions
the kernel calls and verifies, for every 64 x 16 tile of a box, that every ring element a marched
node reads is written exactly once from the right padded-plane element, that source offsets are
16-byte aligned and inside the plane's record (or the out-of-range offset), that no pair straddles a
staged row, no piece leaves its slot, and that the 5-slot schedule never overwrites a live plane."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "st_dma_map_check.cpp")

# (nx, ny, nz, kc, pad_align): the GPU test's shapes (one z-chunk, and chunks of odd / even length) in
# the default padded layout (pitch a multiple of 16 nodes, x 8 mod 16: rows shifted by one double) and
# in the two others (x 16-byte aligned, pitch nx + 2 or rounded); a two-rank x split's local box; a
# box whose last row ends its plane (nx + 2 a multiple of 16: the shifted record's last pair reads
# the double behind the plane); the 256^3 headline's tiles with its chunk length
SHAPES = [(48, 48, 48, 48, 1), (48, 48, 48, 10, 0), (70, 20, 12, 12, 1), (70, 20, 12, 3, 2), (38, 22, 9, 9, 1),
          (38, 22, 9, 2, 0), (37, 37, 37, 37, 1), (258, 5, 4, 4, 1), (254, 30, 4, 4, 1), (256, 256, 256, 64, 1),
          (256, 256, 256, 7, 0)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("st_dma") / "st_dma_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-o", exe, SRC], check=True, capture_output=True, text=True)
    return exe


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_st_dma_staging_map(checker, shape):
    out = subprocess.run([checker, *map(str, shape)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failures"), out.stdout + out.stderr


def test_st_dma_checker_rejects_odd_pitch(checker):
    """An odd row pitch (37^3 in the unrounded layout: 39 nodes) is not eligible, the host falls back to
    k_spmv_st: the checker refuses it."""
    out = subprocess.run([checker, "37", "37", "37", "37", "0"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, out.stdout + out.stderr
