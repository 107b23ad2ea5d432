"""The host planner (kg_instance_segmentation_amd/routes.py) on its own: every threshold at both sides of its edge, and the glue of the two oracles
(oracle/densecases.py `plan`, oracle/segcases.py `plan_routes`) against the planner's answer for every dense case and every box population.  (no GPU needed;
what the LIBRARY does with a launch is asserted in tests/test_dense_routes_cpu.py, tests/test_seg_routes_cpu.py and their GPU halves)"""
import ast
import os

import pytest

from kg_instance_segmentation_amd import routes
from oracle import densecases as dc, segcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense(N, OH, OW, k=3, stride=1, cin_pad=64, cout=64, w_rows=None, xP=1, wP=1, yP=1, rP=1, transposed=False, rows_out=True, res=False, mask=False,
          oscale=False, tile=0, tiny=True, armed=False, xcols=None):
    return routes.dense_conv(N * OH * OW, N, OH, OW, k, stride, k // 2, cin_pad, cin_pad if xcols is None else xcols, cout if w_rows is None else w_rows,
                             xP, wP, yP, rP, cout, transposed, rows_out, res, mask, oscale, True, tile, tiny, armed)


def test_module_imports_nothing_but_math_and_functools():
    with open(os.path.join(ROOT, "kg_instance_segmentation_amd", "routes.py")) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add("." * node.level + (node.module or ""))
    assert names == {"math", "functools"}


def test_dense_tiny_thresholds():
    assert (routes.CONV_TINY_WGS, routes.CONV_TINY_TILES) == (96, 384)
    # 16 x 8 images, 64 couts: one 16 x 32 workgroup and two 64-pixel tiles per image
    assert dense(95, 16, 8) == ("tiny", "kg_conv2d_igemm")                      # 95 workgroups < 96, 190 tiles
    assert dense(96, 16, 8)[0] == "halo"                                        # 96 workgroups
    assert dense(95, 16, 8, tiny=False)[0] == dense(95, 16, 8, tile=3)[0] == "halo"
    assert dense(1, 128, 192) == ("tiny", "kg_conv2d_igemm")                    # 48 workgroups, 24576 pixels = 384 tiles
    assert dense(1, 160, 154)[0] == "halo"                                      # 50 workgroups, 24640 pixels = 385 tiles
    assert dense(10, 8, 8)[0] == "halo"                                         # 10 workgroups == 10 tiles: nothing to split
    assert dense(10, 8, 9)[0] == "tiny"                                         # 10 workgroups < 12 tiles
    # the regular kernel that would serve the launch sets the workgroup count: 256 x 128 gather tiles for a strided conv
    assert dense(1, 64, 64, stride=2)[0] == "tiny" and dense(1, 64, 64, stride=2, cout=128)[0] == "tiny"      # 16 wgs, 64 / 128 tiles
    assert dense(1, 64, 64, k=7)[0] == "halo" and dense(1, 64, 64, rows_out=False)[0] == "halo"               # 49 taps / fp32 export: never
    assert dense(1, 64, 64, cin_pad=8, stride=2)[0] == "igemm"                                               # no 64-channel chunks


def test_ragged_fill_thresholds():
    assert routes.RAGGED_FILL * 20 * 512 == 3584 and routes.RAGGED_FILL * 20 * 256 == 1792

    def conv3(M, tiles=20, cin_pad=64, xcols=64):
        return routes.ragged_conv(3, M, tiles, cin_pad, xcols, 64, False, True, True)
    assert conv3(3583) == "gather" and conv3(3584) == "halo"
    assert conv3(3584, tiles=0) == conv3(3584, cin_pad=8, xcols=8) == conv3(3584, cin_pad=128) == "gather"      # no table / thin / narrow input
    assert not routes.ragged_wgrad_halo(3, 1791, 20) and routes.ragged_wgrad_halo(3, 1792, 20)
    assert not routes.ragged_wgrad_halo(1, 1792, 20) and not routes.ragged_wgrad_halo(3, 1792, None)
    # the weight gradient of a ragged launch: the halo kernel when it is handed the table, else the gather kernel
    assert routes.wgrad(1792, None, 0, 0, 3, 1, 1, 64, 64, 64, 64, 1, 1, 2, True, False, 20, True)[0] == "halo"
    assert routes.wgrad(1791, None, 0, 0, 3, 1, 1, 64, 64, 64, 64, 1, 1, 2, True, False, None, True)[0] == "gather"


def test_1x1_thresholds():
    def c(cin_pad, w_rows, **kw):
        a = dict(k=1, stride=1, pad=0, xcols=cin_pad, planed=False, rows_out=True, same_rows=True)
        a.update(kw)
        return routes.can_1x1(a["k"], a["stride"], a["pad"], cin_pad, a["xcols"], w_rows, a["planed"], a["rows_out"], a["same_rows"])
    assert c(128, 64) and c(128, 65) and c(192, 64) and not c(192, 65)          # compute-heavy: K >= 192 and more than 64 weight rows
    assert c(1024, 64) and not c(1088, 64) and c(64, 256) and not c(8, 64) and not c(96, 64)
    for kw in (dict(planed=True), dict(k=3), dict(stride=2), dict(pad=1), dict(rows_out=False), dict(same_rows=False), dict(xcols=64)):
        assert not c(128, 64, **kw), kw
    for kw in (dict(xP=2), dict(wP=2), dict(yP=2), dict(res=True, rP=2)):      # any operand on two planes
        assert dense(2, 20, 20, k=1, cin_pad=128, cout=256, tiny=False, **kw)[0] == "igemm", kw
    assert dense(2, 20, 20, k=1, cin_pad=128, cout=256, tiny=False) == ("1x1", "kg_conv1x1")
    assert dense(2, 20, 20, k=1, cin_pad=128, cout=256, tiny=False, oscale=True)[0] == "igemm"
    assert dense(2, 20, 20, k=1, cin_pad=192, cout=256, tiny=False)[0] == "igemm"
    assert routes.ragged_conv(1, 700, 0, 128, 128, 256, False, True, True) == "1x1"
    assert routes.ragged_conv(1, 700, 0, 128, 128, 256, True, True, True) == "gather"


def entry(cout=64, cin_pad=64, k=3, xP=1, wP=1, yP=1, rP=1, rows_out=True, res=False, mask=False, flip=False, oscale=False, armed=False, ragged=False,
          t8=False, t16=False):
    return routes.halo_entry(k, cin_pad, cout, xP, wP, yP, rP, rows_out, res, mask, flip, oscale, armed, ragged, t8, t16)


def test_weight_stationary_entry():
    ws = dict(xP=2, wP=2, yP=2)
    assert entry(**ws) == entry(**dict(ws, yP=1)) == "kg_conv3x3_ws"
    assert entry(**dict(ws, yP=3)) == "kg_conv2d_halo"
    assert entry(**ws, armed=True) == "kg_conv2d_halo"
    assert entry(**ws, ragged=True, t8=True, t16=True) == "kg_conv3x3_ws"
    assert entry(**ws, ragged=True, t16=True) == "kg_conv2d_halo"
    for kw in (dict(res=True, rP=2), dict(mask=True), dict(flip=True), dict(oscale=True), dict(rows_out=False), dict(cout=128), dict(cin_pad=128), dict(k=7),
               dict(xP=3, wP=3), dict(wP=1)):
        assert entry(**dict(ws, **kw)) == "kg_conv2d_halo", kw
    routes.USE_WS = False
    try:
        assert entry(**ws) == "kg_conv2d_halo"
    finally:
        routes.USE_WS = True
    assert dense(2, 21, 37, tiny=False, **ws) == ("halo", "kg_conv3x3_ws") and dense(2, 21, 37, tiny=False, armed=True, **ws) == ("halo", "kg_conv2d_halo")


def test_c64_entry():
    assert entry() == entry(cout=200) == entry(flip=True, res=True, mask=True) == "kg_conv3x3_c64"
    assert entry(ragged=True, t16=True) == "kg_conv3x3_c64" and entry(ragged=True, t8=True) == "kg_conv2d_halo"
    for kw in (dict(xP=2), dict(wP=2), dict(yP=2), dict(res=True, rP=2), dict(oscale=True), dict(rows_out=False), dict(cin_pad=128), dict(k=7)):
        assert entry(**kw) == "kg_conv2d_halo", kw


def test_dense_weight_gradient():
    def wg(cin, k, stride=1, N=2, one=True, acc=False, cout=64, H=32, W=32, xP=1, dP=1, bias=False):
        OH, OW = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        return routes.wgrad(N * OH * OW if N else OH * OW, N, H, W, k, stride, k // 2, cin, cout, routes.round_up(cin, 8), routes.round_up(cout, 8), xP, dP, 0,
                            one, acc, None, bias)
    assert wg(4, 3)[0] == "halo" and wg(4, 5)[0] == "im2col" and wg(4, 7)[0] == "im2col" and wg(3, 7, stride=2)[0] == "im2col"
    assert wg(8, 3)[0] == wg(8, 7)[0] == "halo" and wg(8, 5)[0] == "gather"
    assert wg(4, 7, one=False)[0] == wg(4, 7, acc=True)[0] == "halo" and wg(4, 7, N=None)[0] == "gather"
    assert wg(64, 3, stride=2)[0] == "gather" and wg(64, 1)[0] == "gather"
    # halo: cit / nblk / fused bias (7x7 with at most 16 couts and a bias: 32 input channels per workgroup; planed operands: no fused bias)
    assert wg(64, 3, cout=200)[1:5] == (64, 200, 64, 4) and wg(192, 7)[3:5] == (16, 12)
    assert wg(64, 7, cout=5, bias=True)[3:] == (32, 2, wg(64, 7, cout=5, bias=True)[5], True)
    assert wg(64, 7, cout=5)[3] == 16 and wg(64, 7, cout=5, bias=True, xP=2, dP=2)[3::3] == (16, False)
    assert wg(64, 3, bias=True)[6] is True and wg(64, 3, stride=2, bias=True)[6] is False
    # pixel splits: the ring tiles with the LDS transpose reads on, 64 x 64 tiles without them
    M = 2 * 32 * 32
    assert wg(256, 1, cout=512)[5] == routes.wgrad_splits(M, 256, 512, 1, 512 * 256) == 10
    routes.WGRAD_TR[0] = False
    try:
        assert routes.wgrad_splits(M, 256, 512, 1, 512 * 256) == 8
    finally:
        routes.WGRAD_TR[0] = True
    assert routes.vplanes(1, 1) == 1 and routes.vplanes(2, 2) == 3 and routes.vplanes(3, 3) == 6 and routes.vplanes(2, 1) == 2


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.op in ("fwd", "dgrad", "wgrad")], ids=lambda c: c.name)
def test_dense_oracle_reports_the_planners_answer(case):
    c, P = case, case.P
    kind, key, S = dc.plan(c)
    if c.op == "wgrad":
        got = routes.wgrad(c.N * c.OH * c.OW, c.N, c.H, c.W, c.k, c.stride, c.pad, c.cin, c.cout, dc.round_up(c.cin, 8), dc.round_up(c.cout, 8), P, P, 0, True,
                           False, None, bool(c.bias_out))
        assert got[0] == kind == c.kind
        assert key.entry == ("kg_conv2d_wgrad_halo" if kind == "halo" else "kg_conv2d_wgrad")
        if kind != "im2col":
            assert got[5] == S and (key.split is True) == (S > 1) and ("dbias" in key.epi) == got[6]
        return
    fwd = c.op == "fwd"
    cin, cout, OH, OW = (c.cin, c.cout, c.OH, c.OW) if fwd else (c.cout, c.cin, c.H, c.W)
    cin_pad = dc.round_up(cin, 8)
    got = routes.dense_conv(c.N * OH * OW, c.N, OH, OW, c.k, c.stride, c.pad, cin_pad, cin_pad, cout, P, P, P, P if c.res else 1, cout, not fwd,
                            not c.f32 if fwd else True, c.res, c.mask, c.oscale, True, 0, c.tiny, c.armed)
    assert got == (kind, key.entry) and kind == c.kind


def seg_launch(pas, l, conv):
    """(cin_pad, cout) of a ragged conv of the seg branch from its name, pass and level (seg.SegBranch.run_forward / _run_backward)"""
    cin, cout, ccat = (64, 64 if conv == "seg_head.0" else 1, 64) if conv.startswith("seg_head") else sc.SKIP[l]
    cin = ccat if conv.endswith("cat_conv.0") else cin
    return (dc.round_up(cout, 8), cin) if pas == "bwd" else (dc.round_up(cin, 8), cout)


@pytest.mark.parametrize("policy", sorted(sc.POLICY_PLANES))
@pytest.mark.parametrize("name", sc.NAMES)
def test_seg_oracle_reports_the_planners_answer(name, policy):
    p, routes_ = sc.plan_routes(sc.populations()[name], policy)
    seen = 0
    for pas, l, conv, tag, info in routes_:
        ent = tag.split("/")[0]
        if ent == "kg_conv2d_wgrad_halo" or ent == "kg_conv2d_wgrad":
            want = routes.ragged_wgrad_halo(3 if "tiles16" in info else 1, info["M"], info.get("tiles16"))
            assert (ent == "kg_conv2d_wgrad_halo") == want, (pas, l, conv, tag)
        elif ent in ("kg_conv3x3_ws", "kg_conv3x3_c64", "kg_conv2d_halo", "kg_conv2d_igemm", "kg_conv1x1"):
            P = sc.POLICY_PLANES[policy][0 if pas == "fwd" else 1]
            cin_pad, cout = seg_launch(pas, l, conv)
            k = 3 if "tiles32" in info else 1
            route = routes.ragged_conv(k, info["M"], info.get("tiles32", 0), cin_pad, cin_pad, cout, P > 1, True, True)
            if route == "halo":
                t8 = pas == "fwd" and l == 0
                assert ent == routes.halo_entry(3, cin_pad, cout, P, P, P, 1, True, False, pas == "bwd", pas == "bwd", False, False, True, t8, True), (pas, l, conv, tag)
            else:
                assert ent == {"1x1": "kg_conv1x1", "gather": "kg_conv2d_igemm"}[route], (pas, l, conv, tag)
        else:
            continue
        seen += 1
    assert seen or p.top < 0
