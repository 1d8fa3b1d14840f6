"""conv3x3_chunk.hip without a GPU: the exported plan rule pinned against the table it was fitted on (profiles/conv3x3_chunk_ab.txt),
the header / Makefile / binding, and the host replay of the kernel's stage and buffer hand-over schedule."""
import os
import shutil
import subprocess

import pytest

from cfpnet_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the model's eleven 3x3 stride-1 convolutions on more than 64 input channels at batch 8: (layer, M, Cin, Cout, tile alone, tile in flight)
MODEL_SHAPES = [
    ("decoder.up3.a", 153600, 168, 64, 1, 1),
    ("decoder.up2.a", 38400, 312, 128, 1, 1),
    ("decoder.up1.a", 9600, 392, 256, 1, -1),
    ("decoder.up1.b", 9600, 256, 256, 1, -1),
    ("decoder.up2.b", 38400, 128, 128, 1, 1),
    ("dapm128.conv1 a", 9600, 256, 128, -1, 1),
    ("dapm128.conv1 b", 9600, 256, 128, -1, 1),
    ("dapm64.conv1 a", 38400, 128, 64, 1, 1),
    ("dapm64.conv1 b", 38400, 128, 64, 1, 1),
    ("dapm128.conv2 a", 9600, 128, 128, -1, 1),
    ("dapm128.conv2 b", 9600, 128, 128, -1, 1),
]


def want(M, Cin, Cout, in_flight):
    """The measured rule, restated: tile 1 (64 channels x 8 x 16 pixels, three workgroups per CU) from 30 000 to 200 000 pixels; around
    9 600 pixels the outputs wider than 128 channels alone and the others in flight; nothing else moves."""
    if Cin <= 64 or Cin % 8 or Cout % 8:
        return -1
    if 30000 <= M < 200000:
        return 1
    if 8000 <= M < 12000:
        return 1 if (Cout > 128) != (in_flight > 1) else -1
    return -1


def test_symbol_header_makefile_and_binding():
    lib = hip.load()
    assert hasattr(lib, "cfp_conv3x3_chunk_variant")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_conv3x3_chunk_variant(int M, int Cin, int Cout, int in_flight);" in text
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert "conv3x3_chunk.hip" in mk and "conv3x3_chunk.o" in mk


@pytest.mark.parametrize("name,M,Cin,Cout,alone,inflight", MODEL_SHAPES)
def test_the_models_shapes_take_what_the_summary_says(name, M, Cin, Cout, alone, inflight):
    lib = hip.load()
    assert lib.cfp_conv3x3_chunk_variant(M, Cin, Cout, 1) == alone, name
    assert lib.cfp_conv3x3_chunk_variant(M, Cin, Cout, 4) == inflight, name


def test_rule_over_a_grid():
    lib = hip.load()
    for M in (1200, 4800, 7999, 8000, 9600, 11999, 12000, 19200, 29999, 30000, 38400, 76800, 153600, 199999, 200000, 614400):
        for Cin in (8, 32, 64, 68, 72, 128, 168, 256, 312, 392, 512):
            for Cout in (16, 32, 64, 128, 136, 256, 512):
                for fl in (0, 1, 2, 4):
                    assert lib.cfp_conv3x3_chunk_variant(M, Cin, Cout, fl) == want(M, Cin, Cout, fl), (M, Cin, Cout, fl)


def test_never_for_64_input_channels_or_fewer():
    lib = hip.load()
    for Cin in range(8, 65, 8):
        for M in (9600, 38400, 153600, 614400):
            for Cout in (32, 64, 128, 256):
                assert lib.cfp_conv3x3_chunk_variant(M, Cin, Cout, 1) == -1 and lib.cfp_conv3x3_chunk_variant(M, Cin, Cout, 4) == -1


def test_plan_reports_the_kernel_and_the_switch_turns_it_off():
    import ctypes
    lib = hip.load()

    def plan(M, Cout, Cin, KH=3, stride=1, rpb=0):
        v, s = ctypes.c_int(0), ctypes.c_int(0)
        lib.cfp_conv2d_plan(M, Cout, KH * KH * Cin, KH, stride, hip.BF16, rpb, 8, ctypes.byref(v), ctypes.byref(s))
        return v.value

    assert plan(153600, 64, 168) == 601 and plan(38400, 128, 312) == 601
    assert plan(9600, 128, 256) < 600                                   # alone: the direct kernel keeps it
    assert plan(38400, 128, 312, stride=2) < 600 and plan(38400, 128, 312, rpb=4800) < 600 and plan(38400, 128, 64) < 600
    assert plan(38400, 128, 312, KH=1) < 600
    try:
        lib.cfp_debug_set(40, 0)
        assert plan(153600, 64, 168) < 600 and lib.cfp_conv3x3_chunk_variant(153600, 168, 64, 4) == -1
        lib.cfp_debug_set(40, 2)
        assert plan(9600, 128, 256) == 600 and plan(9600, 64, 256) == 601 and plan(9600, 64, 64) < 600
    finally:
        lib.cfp_debug_set(40, 1)


def test_hand_over_schedule_replayed_on_the_host(tmp_path):
    """tools/probes/chunk16_schedule.cpp: for 1 ... 7 and 12 chunks no weight stage and no halo content is written while a reader of the
    previous content can still be in front of the barrier, and the three deliberately wrong schedules are caught."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    args = []
    if cxx is None:
        cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        args = ["-x", "c++"]
    exe = str(tmp_path / "chunk16_schedule")
    subprocess.check_call([cxx, "-std=c++17", "-O1", *args, os.path.join(ROOT, "tools", "probes", "chunk16_schedule.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schedule ok" in out.stdout and "HAZARD" not in out.stdout
