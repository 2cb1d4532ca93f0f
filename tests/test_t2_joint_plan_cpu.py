"""CPU: the host's share of Tier-2 on the device for sub-sampled images, surfaces and packed frames.

tests/c/t2_joint_units.cpp is a stand-alone program over t2_device_plan_joint and joint_tile_classes (grok_amd/csrc/t2_order.h), built
with g++ together with geometry.cpp and t2_writer.cpp: for 4:2:0, 4:2:2, the factors (1,1),(2,1),(1,2) and a four-component
(1,1),(2,2),(2,2),(1,1) image over the five progression orders it checks that the joint plan's packets are packet_order's, that every
row lies in exactly one packet, that row0 / first_block address the host writer's row order and u_words / h_bytes bound the host
header writer's output for random lengths (the writer's own PLT says how long each packet's header came out), that the tile classes of
ragged layouts with an image offset hold tiles of equal sequences and plans and differ from each other, and that the single-geometry
t2_device_plan is, field by field, the function it replaces.

tests/c/t2_keep_sim.cpp runs KK (grok_amd/csrc/kernels_t2keep.hip) as host C++ against tests/c/hip_sim, thread after thread, in heap
blocks of exactly the buffers' sizes: rows and bytes against a plain loop.

Both run under AddressSanitizer and UBSan.  (The GPU runs: tests/test_gpu_t2_joint.py.)"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "grok_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_joint_plan_and_tile_classes_under_sanitizers(tmp_path):
    exe = str(tmp_path / "t2_joint_units")
    subprocess.check_call(["g++"] + SAN + ["-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", os.path.join(HERE, "c", "t2_joint_units.cpp"),
                                           os.path.join(CSRC, "geometry.cpp"), os.path.join(CSRC, "t2_writer.cpp"), "-o", exe, "-lpthread"])
    out = run(exe)
    assert out.startswith("ok: ") and int(out.split()[1]) > 100000, out[-400:]


def test_keep_kernel_thread_by_thread_under_sanitizers(tmp_path):
    exe = str(tmp_path / "t2_keep_sim")
    subprocess.check_call(["g++", "-x", "c++"] + SAN + ["-Wno-attributes", "-I" + os.path.join(HERE, "c", "hip_sim"),
                                                       os.path.join(HERE, "c", "t2_keep_sim.cpp"), "-o", exe])
    out = run(exe)
    assert out.startswith("ok: ") and int(out.split()[1]) == 144, out[-400:]      # (12 batches in 6 sequences, 6 repeats, 2 alignments)
