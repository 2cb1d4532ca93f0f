"""CPU: the two surface kernels' own code (grok_amd/csrc/kernels_surface.hip) as host C++ -- tests/c/surface_kernels_sim.cpp compiles the
file against a few lines that stand in for the HIP runtime (tests/c/hip_sim) and runs every launch thread after thread, under
AddressSanitizer and UBSan, in heap blocks of exactly the surface's and the unit planes' sizes.  Every path of KS and KD -- the
shifting row move, four two-byte samples out of a 16-byte line, the merged partner pairs of one- and two-byte samples, the
sample-by-sample fallbacks on odd addresses and pitches -- against plain index arithmetic, at every alignment of the first sample:
a sample computed wrong, a byte written that is no sample, an access outside the surface or off its alignment fails here, without a
GPU.  (The GPU runs of the same cases: tests/test_gpu_surface_msb.py.)"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_surface_kernels_thread_by_thread_under_sanitizers(tmp_path):
    exe = str(tmp_path / "surface_kernels_sim")
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-attributes", "-I" + os.path.join(HERE, "c", "hip_sim"), os.path.join(HERE, "c", "surface_kernels_sim.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.startswith("ok: ") and int(run.stdout.split()[1]) > 10000, run.stdout[-400:]
