"""No GPU: the host statements of the instance-result semantics (instances.label_map_host / table_host / overlay_host, the run-length
functions) on literal cases and on the reference's own apply_mask output (tests/golden/overlay.npz, tools/gen_instances_goldens.py), and
the host-side argument validation of kg_instance_labels / kg_instance_overlay.  Every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

from kg_instance_segmentation_amd import _lib, bitmasks, inference, instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid(rows):
    return np.array(rows, np.int32)


def two_overlapping():
    m = np.zeros((2, 4, 5), np.uint8)
    m[0, 0:2, 0:3] = 1
    m[1, 1:3, 1:4] = 1
    return m


def test_two_overlapping_masks():
    m = two_overlapping()
    assert np.array_equal(instances.label_map_host(m), grid([[1, 1, 1, 0, 0],
                                                             [1, 1, 1, 2, 0],
                                                             [0, 2, 2, 2, 0],
                                                             [0, 0, 0, 0, 0]]))
    t = instances.table_host(m)
    assert t.dtype == np.int64
    assert np.array_equal(t, [[6, 6, 0, 0, 2, 3, 3, 6],
                              [6, 4, 1, 1, 3, 4, 7, 9]])


def test_priority_reversed():
    m = two_overlapping()
    assert np.array_equal(instances.label_map_host(m, priority=[1, 0]), grid([[1, 1, 1, 0, 0],
                                                                              [1, 2, 2, 2, 0],
                                                                              [0, 2, 2, 2, 0],
                                                                              [0, 0, 0, 0, 0]]))
    assert np.array_equal(instances.table_host(m, priority=[1, 0]), [[6, 4, 0, 0, 2, 3, 1, 3],
                                                                    [6, 6, 1, 1, 3, 4, 9, 12]])
    with pytest.raises(ValueError):
        instances.label_map_host(m, priority=[1, 1])


def test_hidden_and_empty_masks():
    m = np.zeros((3, 4, 5), np.float32)
    m[0, 0:3, 1:4] = 1
    m[1, 1, 2] = 1                         # fully under mask 0
    lab = instances.label_map_host(m)
    assert lab.dtype == np.int32
    assert np.array_equal(lab, grid([[0, 1, 1, 1, 0],
                                     [0, 1, 1, 1, 0],
                                     [0, 1, 1, 1, 0],
                                     [0, 0, 0, 0, 0]]))
    assert np.array_equal(instances.table_host(m), [[9, 9, 0, 1, 3, 4, 9, 18],
                                                    [1, 0, 0, 0, 0, 0, 0, 0],
                                                    [0, 0, 0, 0, 0, 0, 0, 0]])
    # ids are values: any int32 passes through
    assert np.array_equal(np.unique(instances.label_map_host(m, ids=[-7, 5, 2 ** 31 - 1])), [-7, 0])
    assert instances.label_map_host(np.zeros((0, 4, 5), np.uint8)).tolist() == np.zeros((4, 5), int).tolist()
    assert instances.table_host(np.zeros((0, 4, 5), np.uint8)).shape == (0, 8)


def test_rle_example():
    runs = instances.rle_encode(grid([[1, 0, 0], [1, 1, 0], [0, 1, 0]]))
    assert list(runs) == [1]
    assert runs[1].dtype == np.int64 and np.array_equal(runs[1], [[1, 2], [5, 2]])
    assert instances.rle_string(runs[1]) == "1 2 5 2"
    assert np.array_equal(instances.rle_decode(runs[1], 3, 3), [[1, 0, 0], [1, 1, 0], [0, 1, 0]])


def seeded_masks(n, H, W, seed, smax=12):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(1, smax + 1), rng.integers(1, smax + 1)
        m[k] = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if k % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return m


def test_rle_round_trip():
    m = seeded_masks(9, 37, 70, 3)
    lab = instances.label_map_host(m)
    runs = instances.rle_encode(lab, ids=range(1, 11))
    assert list(runs) == list(range(1, 11))
    assert runs[10].shape == (0, 2) and runs[10].dtype == np.int64            # an id absent from the map
    assert instances.rle_string(runs[10]) == ""
    present = [i for i in range(1, 10) if (lab == i).any()]
    assert len(present) >= 5
    for i in range(1, 10):
        r = runs[i]
        assert np.array_equal(instances.rle_decode(r, 37, 70), lab == i)
        assert np.all(r[:, 1] >= 1) and np.all(r[1:, 0] > r[:-1, 0] + r[:-1, 1])     # ascending, maximal runs
    assert np.array_equal(instances.rle_decode(instances.rle_encode(lab), 37, 70), lab)
    assert sorted(instances.rle_encode(lab)) == present


def golden_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "overlay.npz"))
    for name in sorted({k.split(".")[0] for k in z.files}):
        image = z[f"{name}.image"]
        masks = np.unpackbits(z[f"{name}.bits"], axis=-1, bitorder="little")[:, :, :image.shape[1]]
        yield name, image, masks, z[f"{name}.colors"], float(z[f"{name}.alpha"]), z[f"{name}.out"]


def test_overlay_host_equals_reference():
    seen = {}
    for name, image, masks, colors, alpha, want in golden_cases():
        seen[name] = (image.shape[:2], len(masks), int(masks.sum(0).max()))
        got = instances.overlay_host(image, masks, colors, alpha)
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        assert not np.array_equal(want, image)
    assert seen["small"][:2] == ((37, 70), 9) and seen["wide"][:2] == ((64, 128), 70)
    assert max(s[2] for s in seen.values()) >= 5                            # a pixel under at least five masks
    e = next(c for c in golden_cases() if c[0] == "edge")
    assert (e[3] == 0.0).any() and ((e[3] < 1.0) & (e[3] > 1.0 - 1e-9)).any()


@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    lib = ctypes.CDLL(build.build())
    lib.kg_last_error.restype = ctypes.c_char_p
    for name in ("kg_instance_labels", "kg_instance_overlay"):
        getattr(lib, name).argtypes = _lib._SIGS[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def test_entry_points_validate_on_the_host(lib):
    H, W, n = 4, 5, 3
    ld = bitmasks.ld_words(H, W)
    buf = (ctypes.c_char * 4096)()                         # stands for every device buffer: a failed check returns before any HIP call
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def rs(*v):
        return (ctypes.c_int * len(v))(*v)

    def labels(words=p, ld_words=ld, n=n, row_start=rs(0, 1, 3), nimg=2, H=H, W=W, out=p):
        return lib.kg_instance_labels(words, ld_words, n, row_start, nimg, H, W, None, out, p, None)

    def overlay(words=p, ld_words=ld, n=n, row_start=rs(0, 1, 3), nimg=2, H=H, W=W, image=p, colors=p, alpha=0.8):
        return lib.kg_instance_overlay(image, words, ld_words, n, row_start, nimg, H, W, colors, alpha, p, None)

    bad = [dict(words=None), dict(row_start=None), dict(ld_words=ld + 1), dict(ld_words=ld - 2), dict(row_start=rs(0, 2, 1)),
           dict(row_start=rs(1, 2, 3)), dict(row_start=rs(0, 1, 2)), dict(row_start=rs(0, 1, 4)), dict(H=0), dict(W=-1), dict(n=-1), dict(nimg=0),
           dict(words=ctypes.c_void_p(p.value + 8)), dict(nimg=2, H=1 << 16, W=1 << 15, ld_words=1 << 26)]
    for fn, name, more in ((labels, b"kg_instance_labels", [dict(out=None)]),
                           (overlay, b"kg_instance_overlay", [dict(image=None), dict(colors=None), dict(alpha=1.5), dict(alpha=-0.1)])):
        for kw in bad + more:
            assert fn(**kw) != 0, (name, kw)
            assert name in lib.kg_last_error(), (name, kw, lib.kg_last_error())


def test_cpu_tensors_are_refused():
    m = bitmasks.BitMasks(torch.zeros(2, bitmasks.ld_words(4, 5), dtype=torch.int64), 4, 5)
    with pytest.raises(_lib.KGLibraryError):
        instances.label_map(m)
    with pytest.raises(_lib.KGLibraryError):
        instances.overlay(np.zeros((4, 5, 3), np.uint8), m, np.zeros((2, 3)))
    with pytest.raises(_lib.KGLibraryError):
        inference.predict_instances(None, torch.zeros(1, 3, 64, 64))
    with pytest.raises(_lib.KGLibraryError):
        inference.instances_from_predictions([[m, np.zeros((2, 5), np.float32)]])


def test_product_module_stands_alone():
    src = open(os.path.join(ROOT, "kg_instance_segmentation_amd", "instances.py")).read()
    assert "oracle" not in src
