"""The batched flavour of the shape-specialised build (FKS_SHAPE_BATCHED, fks_specialize.cpp's
Shape.batched), compiled here without a GPU: fks_shapec, the compiler process the library
starts, builds it with the library's options for the four shapes of
test_specialize.py::test_shape_build_compiles_for_every_family.  The code object must hold the
two batch kernels and nothing of the plain module, within the register budgets the library gates
on: 96 VGPRs at five waves per SIMD (128 at the lean block's four), 256 for the small-batch
kernel."""
import os
import re
import subprocess

import pytest

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

SHAPES = [
    ("cfg3_arm", dict(TYPE=0, L=8, J=7, D=7, W=7, G=8, P=512, PAIR=1, LEAN=0), [], 96),
    ("cfg5_dual_arm_lean", dict(TYPE=0, L=17, J=16, D=14, W=14, G=17, P=1088, PAIR=0, LEAN=1), ["-DFKS_WAVES_PER_EU=4"], 128),
    ("se2", dict(TYPE=1, L=1, J=0, D=3, W=3, G=1, P=64, PAIR=0, LEAN=0), [], 96),
    ("se3", dict(TYPE=2, L=1, J=0, D=6, W=12, G=1, P=256, PAIR=0, LEAN=0), [], 96),
]


def kernels_of(notes):
    """{kernel name: {key: value}} of the integer fields in llvm-readelf's metadata note"""
    out, current = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        key, value = m.groups()
        if key == ".agpr_count":  # the first key of a kernel's (sorted) map
            current = {}
        if current is None:
            continue
        if key == ".name" and value.startswith("fks_"):
            out[value] = current
        elif value.isdigit():
            current[key] = int(value)
    return out


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    from fast_kinematic_simulator_amd import build

    src = tmp_path_factory.mktemp("batched_src")
    for name, rel in build.EMBEDDED:
        (src / name).write_bytes(open(os.path.join(build.PKG, rel), "rb").read())
    return build.build_shapec(), src


@pytest.mark.parametrize("name,shape,extra,budget", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapec_builds_the_batched_flavour(sources, tmp_path, name, shape, extra, budget):
    shapec, src = sources
    out = tmp_path / "k.hsaco"
    cmd = [shapec, str(out), str(src), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", *extra,
           "-DFKS_SHAPE_BATCHED=1"] + [f"-DFKS_SHAPE_{k}={v}" for k, v in shape.items()]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    notes = subprocess.run([READELF, "--notes", str(out)], stdout=subprocess.PIPE, text=True, check=True).stdout
    kernels = kernels_of(notes)
    print(name, {k: (v.get(".vgpr_count"), v.get(".agpr_count")) for k, v in kernels.items()})
    lean = shape["LEAN"] != 0
    expected = {"fks_simulate_shaped_pj"} | (set() if lean else {"fks_simulate_shaped_pj_small"})
    # nothing of the plain module (fks_simulate_shaped, fks_check_configs_shaped, fks_simulate_shaped_small)
    assert set(kernels) == expected, sorted(kernels)
    assert not re.search(r"\.name:\s+fks_simulate_shaped\s*$", notes, re.M)
    assert all(len(k) <= 31 for k in kernels)  # a MessagePack fixstr, which kernel_metadata_uint matches
    assert 0 < kernels["fks_simulate_shaped_pj"][".vgpr_count"] <= budget, kernels
    if not lean:
        assert 0 < kernels["fks_simulate_shaped_pj_small"][".vgpr_count"] <= 256, kernels


def test_cpp_program_builds_and_reports_a_missing_device():
    """tests/cpp/shaped_batches_interface_test.cpp (PrepareKernels(robot, batched = true),
    BatchedSpecializationStatus()) compiles with g++ over the public headers; without a GPU the
    factory reports FKS_ERR_NO_DEVICE (exit 3).  tests/test_shaped_batches.py runs it on the GPU."""
    from fast_kinematic_simulator_amd.build import build_shaped_batches_test

    exe = build_shaped_batches_test()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode in (0, 3), (p.stdout, p.stderr)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr


def test_python_binds_the_new_entries():
    from fast_kinematic_simulator_amd import _capi

    bound = {p[0] for p in _capi.PROTOTYPES}
    assert {"fks_prepare_batched_specialization", "fks_set_batched_specialization", "fks_get_batched_specialization"} <= bound
    assert _capi.KERNEL_KINDS[14] == "shaped_path_jobs" and _capi.KERNEL_KINDS[15] == "shaped_path_jobs_small_batch"


def test_plain_flavour_is_unchanged_by_the_batched_sources(sources, tmp_path):
    """Without FKS_SHAPE_BATCHED the shape build holds the plain module's three kernels and none of
    the batch kernels (SE(2), the quickest shape)."""
    shapec, src = sources
    out = tmp_path / "k.hsaco"
    shape = SHAPES[2][1]
    cmd = [shapec, str(out), str(src), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"] + \
          [f"-DFKS_SHAPE_{k}={v}" for k, v in shape.items()]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    notes = subprocess.run([READELF, "--notes", str(out)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert set(kernels_of(notes)) == {"fks_simulate_shaped", "fks_check_configs_shaped", "fks_simulate_shaped_small"}
