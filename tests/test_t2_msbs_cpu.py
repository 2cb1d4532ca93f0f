"""CPU: a packet header under the general zero-bit-plane tag tree -- every block with its own missing_msbs -- as Tier-2 on the device
composes it, and the plan that sizes its scratch.

grok_amd/csrc/t2_bits.h holds the arithmetic (t2_block_bits_msbs, t2_msbs_one_at, t2_tree_nodes) for KT1's msbs instance
(kernels_t2.hip) and for tests/c/t2_msbs_units.cpp alike.  The program sweeps the grids 1x1, 1xn, nx1, 2x2, 3x5, 41x35 and a row of 256
(nine levels), the value patterns constant / random / raster-rising / raster-falling / one leaf apart from all others, and the lengths
0 and 2^k - 1, 2^k, 2^k + 1 up to the device writer's limit; per table the header's pieces, written by the kernel's put_bits into
zeroed words and stuffed by a plain sequential writer, must be the bytes of the host writer (ZbpTree and HeaderBits of t2_writer.cpp,
compiled into the program as it is).  With every leaf at Kmax - 1 the pieces must be t2_block_bits'.  Then the plans: t2_device_plan_msbs
sizes the raw bits and the node bytes for at least what the sweep used, and t2_device_plan still refuses GRK_AMD_CS_BLOCK_MSBS.
It runs under AddressSanitizer and UBSan.  (The GPU runs: tests/test_gpu_t2_msbs.py.)"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_msbs") / "t2_msbs_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-Wno-unused-function", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_msbs_units.cpp"),
                                           os.path.join(CSRC, "geometry.cpp"), "-o", path, "-lpthread"])
    return path


def test_general_tree_headers_and_plans_are_the_host_writers_under_sanitizers(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout, r.stdout[-4000:]
    assert r.stdout.startswith("ok: ") and int(r.stdout.split()[1]) > 100000, r.stdout[-400:]
