"""CPU: the batched post-processing entry points (kg_postproc_batch, kg_skeleton_boxes_batch, kg_nms_batch and their workspace
sizes) are exported and bound, validate their arguments on the host before any HIP call, and the host-side planning of
detect_batch / predict (chunks under a workspace budget, mask rows split by image and output size) is right."""
import ctypes
import subprocess

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib

NEW = ("kg_postproc_batch_workspace_bytes", "kg_postproc_batch", "kg_skeleton_boxes_batch", "kg_nms_batch_workspace_bytes", "kg_nms_batch")
FAKE = ctypes.c_void_p(4096)     # (never dereferenced: every call below fails its host-side checks first)


@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def _err(lib):
    return lib.kg_last_error().decode()


def test_new_symbols_exported_and_bound(lib):
    path = _lib.LIB_PATH
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW:
        assert name in _lib._SIGS and name in _lib.SYMBOLS
        assert name in exported, name
        assert getattr(lib, name).argtypes == _lib._SIGS[name]


def test_batch_workspace_is_n_aligned_slices(lib):
    for H, W in ((64, 64), (256, 256), (96, 160), (1024, 1024)):
        pc = min(5 * H * W, 1 << 16)
        one = lib.kg_postproc_workspace_bytes(H, W, pc, pc)
        assert one % 256 == 0
        for n in (1, 2, 5, 16):
            assert lib.kg_postproc_batch_workspace_bytes(n, H, W, pc, pc) == n * one
    for cap in (1, 100, 32768):
        one = 2 * ((cap * 4 + 255) // 256 * 256) + (cap + 255) // 256 * 256
        assert lib.kg_nms_batch_workspace_bytes(3, cap) == 3 * one
    assert lib.kg_postproc_batch_workspace_bytes(0, 64, 64, 10, 10) == -1
    assert "kg_postproc_batch_workspace_bytes" in _err(lib)
    assert lib.kg_nms_batch_workspace_bytes(0, 10) == -1


def test_postproc_batch_bad_arguments(lib):
    H = W = 64
    pc = 5 * H * W
    need = lib.kg_postproc_batch_workspace_bytes(2, H, W, pc, pc)
    d = ctypes.c_double(0.004)
    call = lib.kg_postproc_batch
    assert call(FAKE, FAKE, FAKE, 0, H, W, d, FAKE, need, pc, pc, FAKE, FAKE, None) != 0 and "image count" in _err(lib)
    assert call(FAKE, None, FAKE, 2, H, W, d, FAKE, need, pc, pc, FAKE, FAKE, None) != 0 and "null pointer" in _err(lib)
    assert call(FAKE, FAKE, FAKE, 2, H, W, d, FAKE, need, pc, pc, None, FAKE, None) != 0 and "null pointer" in _err(lib)
    assert call(FAKE, FAKE, FAKE, 2, H, W, d, FAKE, need - 256, pc, pc, FAKE, FAKE, None) != 0 and "workspace too small" in _err(lib)
    assert call(FAKE, FAKE, FAKE, 2, 0, W, d, FAKE, need, pc, pc, FAKE, FAKE, None) != 0 and "bad size" in _err(lib)
    assert "kg_postproc_batch" in _err(lib)


def test_boxes_and_nms_batch_bad_arguments(lib):
    P4 = ctypes.c_void_p * 4
    sk, ns = P4(*[4096] * 4), P4(*[4096] * 4)
    caps, scales = (ctypes.c_int * 4)(10, 10, 10, 10), (ctypes.c_double * 4)(1, 2, 4, 8)
    fn = lib.kg_skeleton_boxes_batch
    assert fn(0, 4, sk, ns, caps, scales, 1, FAKE, FAKE, 40, None) != 0 and "kg_skeleton_boxes_batch" in _err(lib)
    assert fn(2, 5, sk, ns, caps, scales, 1, FAKE, FAKE, 40, None) != 0
    assert fn(2, 4, sk, ns, caps, scales, 1, None, FAKE, 40, None) != 0 and "null pointer" in _err(lib)
    bad = P4(4096, 4096, 0, 4096)
    assert fn(2, 4, bad, ns, caps, scales, 1, FAKE, FAKE, 40, None) != 0 and "scale 2" in _err(lib)
    nws = lib.kg_nms_batch_workspace_bytes(3, 40)
    fn = lib.kg_nms_batch
    t = ctypes.c_double(0.5)
    assert fn(0, FAKE, FAKE, 40, t, FAKE, nws, FAKE, FAKE, None) != 0 and "kg_nms_batch" in _err(lib)
    assert fn(3, FAKE, None, 40, t, FAKE, nws, FAKE, FAKE, None) != 0 and "null pointer" in _err(lib)
    assert fn(3, FAKE, FAKE, 40, t, FAKE, nws - 1, FAKE, FAKE, None) != 0 and "workspace too small" in _err(lib)


def test_chunk_planner():
    from kg_instance_segmentation_amd.postprocessing import plan_chunks
    assert plan_chunks(5, 100, 10 ** 9) == [(0, 5)]
    assert plan_chunks(5, 100, 200) == [(0, 2), (2, 4), (4, 5)]
    assert plan_chunks(5, 100, 299) == [(0, 2), (2, 4), (4, 5)]
    assert plan_chunks(5, 100, 50) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]      # (at least one image per chunk)
    assert plan_chunks(16, 100, 800) == [(0, 8), (8, 16)]
    assert plan_chunks(1, 100, 1) == [(0, 1)]
    assert plan_chunks(0, 100, 1000) == []
    for n in range(1, 20):
        for budget in (1, 150, 333, 2000):
            ch = plan_chunks(n, 100, budget)
            assert ch[0][0] == 0 and ch[-1][1] == n and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
            assert all(b - a >= 1 and (b - a == 1 or (b - a) * 100 <= budget) for a, b in ch)


def test_image_workspace_bytes_counts_each_size_once(lib):
    from kg_instance_segmentation_amd.postprocessing import caps, image_workspace_bytes
    one = {s: lib.kg_postproc_workspace_bytes(s, s, *caps(s, s)) for s in (64, 32, 16, 8)}
    assert image_workspace_bytes([(64, 64), (32, 32), (16, 16), (8, 8)]) == sum(one.values())
    assert image_workspace_bytes([(64, 64), (64, 64), (16, 16), (8, 8)]) == one[64] + one[16] + one[8]


def test_rows_split_by_image_and_size():
    from kg_instance_segmentation_amd.inference import image_row_ranges, size_groups
    img = np.array([0, 0, 0, 2, 3, 3, 5])
    assert image_row_ranges(img, 6) == [(0, 3), (3, 3), (3, 4), (4, 6), (6, 6), (6, 7)]
    assert image_row_ranges(np.zeros(0, np.int32), 3) == [(0, 0)] * 3
    with pytest.raises(_lib.KGLibraryError):
        image_row_ranges(np.array([1, 0]), 2)
    sizes = [(256, 256), (300, 200), (256, 256), (520, 696), (300, 200)]
    assert size_groups(sizes) == [((256, 256), [0, 2]), ((300, 200), [1, 4]), ((520, 696), [3])]
