"""CPU: the bit string a code-block adds to a packet header, as Tier-2 on the device composes it.

grok_amd/csrc/t2_bits.h holds that arithmetic for KT1 (kernels_t2.hip) and for tests/c/t2_bits_units.cpp alike.  The program sweeps
every tag-tree height the plan admits, every ctz(x | y), the band's first block and the others, and the lengths 2^k - 1, 2^k, 2^k + 1 up
to the device writer's limit; per case the header's pieces, written by the kernel's put_bits into zeroed words and stuffed by a plain
sequential writer, must be the bytes of the host writer's HeaderBits (t2_writer.cpp, compiled into the program as it is).  It runs
under AddressSanitizer and UBSan.

`t2_bits_units parent` runs the same sweep over the arithmetic the header replaced -- the tail as ONE 64-bit value, lengths below
2^29: UBSan reports the shift where the tail first needs more than 64 bits, and the bits written there differ.  (The GPU runs: tests/test_gpu_t2_tables.py.)"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
# (a report of UBSan stops the program where the environment says halt_on_error=1: the sweep; the arithmetic of before is let run on)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
HALT = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t2_bits") / "t2_bits_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-Wno-unused-function", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_bits_units.cpp"),
                                           os.path.join(CSRC, "geometry.cpp"), "-o", path, "-lpthread"])
    return path


def test_block_bit_strings_are_the_host_writers_under_sanitizers(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=HALT)
    assert r.returncode == 0 and "runtime error" not in r.stdout, r.stdout[-4000:]
    assert r.stdout.startswith("ok: ") and int(r.stdout.split()[1]) > 1000000, r.stdout[-400:]


def test_one_64_bit_tail_under_a_29_bit_limit_shifts_out_of_range(exe):
    """The arithmetic before t2_bits.h: at the first case whose tail is 65 bits -- a tree of eight levels (a row of 65 .. 128 blocks)
    and a length of 2^28 -- put_bits shifts by 64 - 65, and the bits it then writes are not the host writer's."""
    r = subprocess.run([exe, "parent"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0
    assert "shift exponent" in r.stdout, r.stdout[-4000:]
    assert "-- tag-tree height 8, block (0, 0), Kmax 1, length 268435456" in r.stdout, r.stdout[-4000:]
