"""CPU: per-instance measurements as measure.py states them in NumPy -- measure_host against a per-pixel Python loop and against
scipy.ndimage where scipy is installed, closed forms for rectangles, rings, single pixels and far-off-origin objects, the band rule, and
the host-side argument validation of kg_label_measure.  Every integer is compared exactly; floats only against closed forms (rtol 1e-12)
or where both sides come from props() on equal integers."""
import ctypes
import math

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib
from kg_instance_segmentation_amd import labelmetrics as lm
from kg_instance_segmentation_amd import measure as ms


def blob_map(H, W, n, seed):
    """A seeded ragged map: ellipses and rectangles with ids 1 .. n painted over each other, some cut by the frame, some touching."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, max(H // 4, 2) + 1), rng.integers(1, max(W // 6, 2) + 1)
        sel = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if i % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        lab[sel & (rng.random((H, W)) < 0.93)] = i                              # ragged: pin-holes and frayed edges
    return lab


def seeded_image(shape, C, dtype, seed):
    top = np.iinfo(dtype).max
    img = np.random.default_rng(seed).integers(0, top + 1, tuple(shape) + (C,)).astype(dtype)
    img.reshape(-1)[::7] = 0
    img.reshape(-1)[3::11] = top
    return img


def brute(lab, n, img=None):
    """The rows of ids 1 .. n by a loop over every pixel, in Python integers."""
    H, W = lab.shape
    C = 0 if img is None else img.shape[2]
    rows = [[0] * (10 + 4 * C) for _ in range(n)]
    seen = [False] * n
    for y in range(H):
        for x in range(W):
            v = int(lab[y, x])
            if not 1 <= v <= n:
                continue
            r = rows[v - 1]
            r[0] += 1; r[1] += y; r[2] += x; r[3] += y * y; r[4] += y * x; r[5] += x * x
            e = 0
            for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if not (0 <= ny < H and 0 <= nx < W):
                    e += 1; r[7] += 1
                elif lab[ny, nx] != v:
                    e += 1; r[8] += int(lab[ny, nx] != 0)
            r[6] += e; r[9] += e > 0
            for c in range(C):
                p = int(img[y, x, c])
                r[10 + 4 * c] += p; r[11 + 4 * c] += p * p
                r[12 + 4 * c] = p if not seen[v - 1] else min(r[12 + 4 * c], p)
                r[13 + 4 * c] = p if not seen[v - 1] else max(r[13 + 4 * c], p)
            seen[v - 1] = True
    return np.array(rows, np.int64).reshape(n, 10 + 4 * C)


SHAPES = [(70, 131), (1, 130), (130, 1)]


def test_columns():
    assert ms.columns(0) == ms.GEOMETRY_COLUMNS and len(ms.GEOMETRY_COLUMNS) == 10
    assert ms.columns(2)[10:] == ("sum_0", "sumsq_0", "min_0", "max_0", "sum_1", "sumsq_1", "min_1", "max_1")
    with pytest.raises(_lib.KGLibraryError):
        ms.columns(5)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("C,dtype", [(0, None), (1, np.uint8), (3, np.uint8), (1, np.uint16), (3, np.uint16)])
def test_measure_host_equals_the_pixel_loop(H, W, C, dtype):
    n = 12
    lab = blob_map(H, W, n, 100 + H)
    img = seeded_image((H, W), C, dtype, 7) if C else None
    want = brute(lab, n, img)
    got = ms.measure_host(lab, n, img)
    assert got.dtype == np.int64 and got.shape == (n, 10 + 4 * C)
    assert np.array_equal(got, want)
    assert (want[:, 0] > 0).sum() >= 3 and want[:, 7].any() and want[:, 8].any()      # objects at the frame, objects that touch
    # jobs given by hand over the whole map measure the same pixels
    jobs = np.array([[0, i, -5, -5, H + 5, W + 5] for i in range(1, n + 1)])
    assert np.array_equal(ms.measure_host(lab, jobs, img), want)
    # a stack: the rows of the images follow each other
    lab2 = blob_map(H, W, 5, 200 + W)
    img2 = None if img is None else np.stack([img, img[::-1, ::-1]])
    both = ms.measure_host(np.stack([lab, lab2]), [n, 5], img2)
    assert np.array_equal(both[:n], want) and np.array_equal(both[n:], brute(lab2, 5, None if img is None else img2[1]))


def test_measure_host_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    H, W, n = 70, 131, 12
    lab = blob_map(H, W, n, 170)
    img = seeded_image((H, W), 2, np.uint16, 9)
    raw = ms.measure_host(lab, n, img)
    idx = np.arange(1, n + 1)
    have = raw[:, 0] > 0
    assert np.array_equal(raw[:, 0], ndi.sum(np.ones_like(lab), lab, idx).astype(np.int64))
    for c in range(2):
        v = img[..., c].astype(np.int64)
        assert np.array_equal(raw[:, 10 + 4 * c], np.asarray(ndi.sum(v, lab, idx)).astype(np.int64))
        assert np.array_equal(raw[:, 11 + 4 * c], np.asarray(ndi.sum(v * v, lab, idx)).astype(np.int64))
        assert np.array_equal(raw[have, 12 + 4 * c], np.asarray(ndi.minimum(v, lab, idx)).astype(np.int64)[have])
        assert np.array_equal(raw[have, 13 + 4 * c], np.asarray(ndi.maximum(v, lab, idx)).astype(np.int64)[have])
    com = np.array(ndi.center_of_mass(np.ones_like(lab), lab, idx[have]))
    assert np.allclose(ms.Measurements(raw).props()["centroid"][have], com, rtol=1e-12, atol=0)


def one(lab, i=1, img=None):
    H, W = lab.shape[-2:]
    return ms.Measurements(ms.measure_host(lab, np.array([[0, i, 0, 0, H, W]]), img))


@pytest.mark.parametrize("h,w", [(5, 9), (12, 3), (7, 7), (1, 6)])
def test_rectangle_closed_forms(h, w):
    lab = np.zeros((30, 40), np.int32)
    lab[4:4 + h, 6:6 + w] = 1
    m = one(lab)
    p = m.props()
    assert m.column("area")[0] == h * w and m.column("edges")[0] == 2 * (h + w) and p["perimeter"][0] == 2 * (h + w)
    assert m.column("edges_border")[0] == 0 and m.column("edges_contact")[0] == 0 and not p["touches_border"][0]
    assert m.column("boundary_pixels")[0] == (h * w - max(h - 2, 0) * max(w - 2, 0))
    assert np.allclose([p["mu_yy"][0], p["mu_xx"][0]], [(h * h - 1) / 12, (w * w - 1) / 12], rtol=1e-12, atol=0) and p["mu_yx"][0] == 0
    assert np.allclose(p["axis_major"][0], 4 * math.sqrt((max(h, w) ** 2 - 1) / 12), rtol=1e-12, atol=0)
    assert np.allclose(p["axis_minor"][0], 4 * math.sqrt((min(h, w) ** 2 - 1) / 12), rtol=1e-12, atol=1e-300)
    assert np.allclose(p["centroid"][0], [4 + (h - 1) / 2, 6 + (w - 1) / 2], rtol=1e-12, atol=0)
    assert np.allclose(p["equivalent_diameter"][0], math.sqrt(4 * h * w / math.pi), rtol=1e-12, atol=0)
    if h != w:
        assert np.allclose(p["orientation"][0], 0.0 if h > w else math.pi / 2, rtol=1e-12, atol=0)       # from the y axis towards x
        big, small = max(h, w) ** 2 - 1, min(h, w) ** 2 - 1
        assert np.allclose(p["eccentricity"][0], math.sqrt(1 - small / big), rtol=1e-12, atol=0)


def test_frame_contact_ring_and_single_pixel():
    lab = np.zeros((20, 30), np.int32)
    lab[0:6, 10:14] = 1                                     # against the top: 4 frame edges
    lab[8:12, 0:5] = 2                                      # against the left: 4
    lab[15:20, 25:30] = 3                                   # in the corner: 5 + 5
    m = ms.Measurements(ms.measure_host(lab, 3))
    assert m.column("edges_border").tolist() == [4, 4, 10] and m.props()["touches_border"].all()
    assert m.column("edges").tolist() == [20, 18, 20] and not m.column("edges_contact").any()
    # two rectangles sharing a side of length 7
    lab = np.zeros((20, 30), np.int32)
    lab[3:10, 4:9] = 1
    lab[3:10, 9:15] = 2
    lab[12:14, 4:6] = 3
    m = ms.Measurements(ms.measure_host(lab, 3))
    assert m.column("edges_contact").tolist() == [7, 7, 0] and m.column("edges").tolist() == [24, 26, 8]
    assert np.allclose(m.props()["contact_fraction"], [7 / 24, 7 / 26, 0], rtol=1e-12, atol=0)
    # a ring counts its inner boundary; the hole's own value touches it as contact when it is another id
    lab = np.zeros((20, 20), np.int32)
    lab[4:13, 5:15] = 1
    lab[7:10, 8:12] = 0
    m = one(lab)
    assert m.column("edges")[0] == 2 * (9 + 10) + 2 * (3 + 4) and m.column("area")[0] == 90 - 12 and m.column("edges_contact")[0] == 0
    lab[7:10, 8:12] = 2
    assert one(lab).column("edges_contact")[0] == 14 and one(lab, 2).column("edges_contact")[0] == 14
    # a single pixel
    lab = np.zeros((5, 5), np.int32)
    lab[2, 3] = 1
    m = one(lab)
    p = m.props()
    assert m.raw[0].tolist() == [1, 2, 3, 4, 6, 9, 4, 0, 0, 1]
    assert p["axis_major"][0] == 0 and p["axis_minor"][0] == 0 and p["eccentricity"][0] == 0 and p["perimeter"][0] == 4
    # a 1 x 1 map: four frame edges
    assert ms.measure_host(np.ones((1, 1), np.int32), 1)[0].tolist() == [1, 0, 0, 0, 0, 0, 4, 4, 0, 1]
    # extreme label values are simply another non-zero value
    lab = np.zeros((5, 6), np.int32)
    lab[2, 2] = 7
    lab[1, 2], lab[3, 2], lab[2, 1] = np.iinfo(np.int32).min, -1, np.iinfo(np.int32).max
    assert one(lab, 7).raw[0, 6:10].tolist() == [4, 0, 3, 1]


def test_area_zero_and_props_nan():
    lab = np.zeros((6, 6), np.int32)
    lab[1:3, 1:3] = 2
    img = np.full((6, 6, 1), 9, np.uint8)
    m = ms.Measurements(ms.measure_host(lab, 2, img))
    assert not m.raw[0].any() and len(m) == 2 and m.channels == 1
    p = m.props()
    for k in ("mu_yy", "axis_major", "axis_minor", "orientation", "contact_fraction", "equivalent_diameter"):
        assert np.isnan(p[k][0]) and not np.isnan(p[k][1]), k
    assert np.isnan(p["centroid"][0]).all() and np.isnan(p["mean"][0, 0]) and np.isnan(p["std"][0, 0])
    assert p["mean"][1, 0] == 9 and p["std"][1, 0] == 0 and m.raw[1, 10:].tolist() == [36, 324, 9, 9]
    empty = ms.Measurements(np.zeros((0, 10), np.int64)).props()
    assert empty["area"].shape == (0,) and empty["centroid"].shape == (0, 2)


def test_far_from_the_origin_the_central_moments_are_those_at_the_origin():
    rng = np.random.default_rng(3)
    blob = rng.random((40, 25)) < 0.7
    ys, xs = np.nonzero(blob)

    def raw_at(oy, ox, v=None):
        y, x = ys.astype(object) + oy, xs.astype(object) + ox
        row = [len(y), y.sum(), x.sum(), (y * y).sum(), (y * x).sum(), (x * x).sum(), 4, 0, 0, 1]
        if v is not None:
            row += [int(v.sum()), int((v.astype(object) ** 2).sum()), int(v.min()), int(v.max())]
        return np.array([row], np.int64)

    near, far = ms.Measurements(raw_at(0, 0)).props(), ms.Measurements(raw_at(32768 - 40, 32768 - 25)).props()
    for k in ("mu_yy", "mu_yx", "mu_xx", "axis_major", "axis_minor", "eccentricity", "orientation"):
        assert near[k][0] == far[k][0], k
    # the float64 shortcut does not: this is why the numerators are formed in integers
    r = raw_at(32768 - 40, 32768 - 25)[0].astype(np.float64)
    shortcut = r[3] / r[0] - (r[1] / r[0]) ** 2
    assert shortcut != near["mu_yy"][0]
    # the same for the variance of a bright 16-bit channel
    v = rng.integers(65000, 65536, len(ys))
    p = ms.Measurements(raw_at(0, 0, v)).props()
    assert np.allclose(p["std"][0, 0], np.std(v.astype(np.float64) - 65000), rtol=1e-12, atol=0)
    assert np.allclose(p["mean"][0, 0], 65000 + np.mean(v.astype(np.float64) - 65000), rtol=1e-12, atol=0)


@pytest.mark.parametrize("cap", [65536, 1000])
def test_bands_add_up_to_the_unsplit_row(cap):
    H, W = 600, 1200
    lab = np.zeros((H, W), np.int32)
    lab[3:590, 5:1105] = 1                                                      # a tall bar, wider than the small cap
    lab[300:320, 400:420] = 0                                                   # a hole
    lab[100:130, 1105:1110] = 2                                                 # a neighbour on its right side
    lab[0:3, 50:60] = 3                                                         # and one above
    img = seeded_image((H, W), 2, np.uint16, 5)
    jobs = np.array([[0, 1, 3, 5, 590, 1105], [0, 2, 100, 1105, 130, 1110], [0, 4, 0, 0, 10, 10]])
    whole = ms.measure_host(lab, jobs, img)
    pieces, owner = ms.split_jobs(jobs, cap)
    assert len(pieces) >= 12 and np.array_equal(np.unique(owner), [0, 1, 2])   # the bar crosses at least nine band boundaries
    if cap == 1000:
        assert (pieces[owner == 0][:, 5] - pieces[owner == 0][:, 3]).max() == 1000 and len(np.unique(pieces[owner == 0][:, 3])) == 2   # row pieces
    got = ms.combine_bands(ms.measure_host(lab, pieces, img), owner, len(jobs))
    assert np.array_equal(got, whole)
    assert whole[0, 0] == 587 * 1100 - 400 and whole[0, 8] == 30 + 10 and whole[0, 6] == 2 * (587 + 1100) + 80 and not whole[2].any()
    # were neighbours read from the box, every band edge would count
    assert ms.measure_host(lab, pieces, img)[owner == 0][:, 6].sum() == whole[0, 6]
    a, b = lm.split_jobs(jobs, cap)
    assert np.array_equal(a, pieces) and np.array_equal(b, owner)                # the band rule is labelmetrics', unchanged


def test_host_refusals():
    lab = np.zeros((4, 5), np.int32)
    with pytest.raises(_lib.KGLibraryError):
        ms.measure_host(lab, 1, np.zeros((4, 5, 5), np.uint8))
    with pytest.raises(_lib.KGLibraryError):
        ms.measure_host(lab, 1, np.zeros((4, 5, 1), np.float32))
    with pytest.raises(_lib.KGLibraryError):
        ms.measure_host(lab, 1, np.zeros((4, 6, 1), np.uint8))
    with pytest.raises(_lib.KGLibraryError):
        ms.measure_host(np.zeros((1, 32769), np.int32), 1)
    with pytest.raises(_lib.KGLibraryError):
        ms.measure_host(lab, np.zeros((2, 5), np.int64))
    with pytest.raises(_lib.KGLibraryError):
        ms.measure(lab, 1)                                                      # a host map: the device route refuses it


def test_instances_have_an_empty_measurements_slot():
    from kg_instance_segmentation_amd import instances, tiling
    a = instances.Instances(None, np.zeros((0, 5), np.float32), None, None)
    b = tiling.TiledInstances(None, np.zeros((0, 5), np.float32), None, None, None, None)
    assert a.measurements is None and b.measurements is None and not hasattr(a, "__dict__")


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def test_entry_is_declared_bound_and_exported(lib):
    assert "kg_label_measure" in _lib.SYMBOLS and hasattr(lib, "kg_label_measure") and len(_lib._SIGS["kg_label_measure"]) == 11


def test_entry_refuses_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_longlong * 4096)()                      # host memory: the entry may never get as far as a launch
    p = ctypes.addressof(buf)
    P, IMG, JOBS, OUT = (ctypes.c_void_p(p + k * 4096) for k in range(4))

    def call(labels=P, nimg=1, H=8, W=8, image=None, channels=0, elem=1, jobs=JOBS, m=3, out=OUT):
        return lib.kg_label_measure(labels, nimg, H, W, image, channels, elem, jobs, m, out, None)

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and "kg_label_measure" in msg and text in msg, (rc, msg)

    err(call(labels=None), "null pointer")
    err(call(jobs=None), "null pointer")
    err(call(out=None), "null pointer")
    err(call(image=IMG), "NULL exactly when channels == 0")
    err(call(channels=3), "NULL exactly when channels == 0")
    err(call(image=IMG, channels=5), "channels 5")
    err(call(image=IMG, channels=-1), "channels -1")
    err(call(image=IMG, channels=3, elem=3), "elem_bytes 3")
    err(call(H=32769), "32768")
    err(call(W=32769), "32768")
    err(call(nimg=0), "bad size")
    err(call(H=0), "bad size")
    err(call(m=-1), "bad size")
    err(call(nimg=3, H=32768, W=32768), "exceeds 2^31 - 1")
    err(call(out=ctypes.c_void_p(p + 3 * 4096 + 4)), "misaligned")
    err(call(labels=ctypes.c_void_p(p + 2)), "misaligned")
    err(call(image=ctypes.c_void_p(p + 4097), channels=1, elem=2), "misaligned")
    assert call(m=0) == 0 and call(m=0, jobs=None, out=None) == 0
    assert call(m=0, image=ctypes.c_void_p(p + 4097), channels=1, elem=1) == 0   # a byte image needs no alignment
