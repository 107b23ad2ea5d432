"""CPU: the text of label_crops_kernel (csrc/crops.hip), compiled as plain C++ by the host compiler with the address and
undefined-behaviour sanitizers and run thread by thread (tests/crops_kernel_host.cpp), equals crops.crops_host on ragged and hostile
job tables -- image indices of -1 and nimg, coefficients and origins of INT_MIN / INT_MAX -- with every buffer an exact-size heap
block: a tap or a store outside its buffer, or an overflow of the position arithmetic, ends the program.  No GPU and no HIP: this checks
the kernel's arithmetic, predicates and store offsets, not the launch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from kg_instance_segmentation_amd import crops as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.iinfo(np.int32)
ONE = 65536
SIZES = [(1, 1), (1, 256), (256, 1), (3, 3), (4, 4), (5, 7), (33, 33), (7, 5), (2, 3), (9, 1), (40, 30)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("crops_kernel_host")
    text, on = [], False
    for line in open(os.path.join(ROOT, "kg_instance_segmentation_amd", "csrc", "crops.hip")):
        if line.startswith("#define KG_CROPS_NEAREST"):
            on = True
        if line.startswith("// ---- host"):
            break
        if on:
            text.append(line)
    assert any("label_crops_kernel" in l for l in text) and not any("hipLaunch" in l for l in text)
    (tmp / "kernel_text.inc").write_text("".join(text))
    exe = str(tmp / "crops_kernel_host")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{tmp}",
                        '-DKERNEL_TEXT="kernel_text.inc"', os.path.join(ROOT, "tests", "crops_kernel_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, tmp


def cases():
    rng = np.random.default_rng(0)
    out = []
    for trial in range(33):
        nimg, H, W, C = int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 5))
        dtype = (np.uint8, np.uint16)[trial % 2]
        lab = rng.integers(0, 4, (nimg, H, W)).astype(np.int32)
        lab[0, 0, 0], lab[-1, -1, -1] = I32.min, I32.max
        img = rng.integers(0, np.iinfo(dtype).max + 1, (nimg, H, W, C)).astype(dtype)
        m = int(rng.integers(1, 8))
        j = np.zeros((m, 10), np.int64)
        j[:, 0], j[:, 1] = rng.integers(-1, nimg + 1, m), rng.choice([0, 1, 2, 3, I32.min, I32.max], m)
        j[:, 2], j[:, 3] = rng.integers(-5, H + 5, m), rng.integers(-5, W + 5, m)
        j[:, 4:] = rng.integers(-2 * ONE, 2 * ONE, (m, 6))
        j = np.where(rng.random((m, 10)) < 0.25, rng.choice([I32.min, I32.max, 0, -1, 1, ONE], (m, 10)), j)     # hostile entries
        out.append(dict(lab=lab, img=None if trial % 3 == 1 else img, jobs=j, size=SIZES[trial % len(SIZES)], flags=int(rng.integers(0, 4)),
                        fill=int(rng.integers(0, 256)), masks=trial % 3 != 2, grid=int(rng.integers(1, 5))))
    return out


def test_kernel_text_on_the_host_equals_the_host_statement(program):
    exe, tmp = program
    todo = cases()
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.int32(len(todo)).tobytes())
        for c in todo:
            nimg, H, W = c["lab"].shape
            C, eb = (1, 1) if c["img"] is None else (c["img"].shape[3], c["img"].dtype.itemsize)
            f.write(np.array([nimg, H, W, C, eb, len(c["jobs"]), *c["size"], c["flags"], c["fill"], c["img"] is not None, c["masks"], c["grid"]], np.int32).tobytes())
            f.write(c["lab"].tobytes())
            if c["img"] is not None:
                f.write(c["img"].tobytes())
            f.write(c["jobs"].astype(np.int32).tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    raw, at, seen = np.fromfile(tmp / "out.bin", np.uint8), 0, 0
    for k, c in enumerate(todo):
        wp, wm = cr.crops_host(c["lab"], c["jobs"], c["img"], c["size"], cr.MODES[c["flags"] & 1], bool(c["flags"] & 2), c["fill"], masks=c["masks"])
        for want in (wp, wm):
            if want is not None:
                got = raw[at:at + want.nbytes].view(want.dtype).reshape(want.shape)
                assert np.array_equal(got, want), k
                at += want.nbytes
                seen += int((want != c["fill"]).sum())
    assert at == len(raw) and seen > 10000
