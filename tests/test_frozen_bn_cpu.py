"""CPU: KGnet.freeze_bn bookkeeping (no kernel runs) and the C ABI of kg_bn_bwd_frozen (header, ctypes table, both libraries)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def model():
    from kg_instance_segmentation_amd import KGnet
    return KGnet.resnet50(pretrained=False)


def _bn_affine(m):
    return {k: m.get_tensor(k) for p in m._bn_prefixes for k in (p + ".weight", p + ".bias")}


def test_default_freezes_all_43_layers_and_their_affine_parameters(model):
    keys = list(model.state_dict().keys())
    assert model.frozen_bn == frozenset() and isinstance(model.frozen_bn, frozenset)
    assert model.freeze_bn() is model
    assert len(model.frozen_bn) == 43 and isinstance(model.frozen_bn, frozenset)
    assert {"bn1", "layer1.0.downsample.1", "layer2.0.bn3", "layer3.5.bn2"} <= model.frozen_bn
    cleared = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert len(cleared) == 86 and set(cleared) == set(_bn_affine(model))
    assert list(model.state_dict().keys()) == keys and len(keys) == 346        # not part of the checkpoint


def test_affine_false_clears_nothing(model):
    model.freeze_bn(affine=False)
    assert len(model.frozen_bn) == 43
    assert all(p.requires_grad for p in model.parameters())


def test_subsets_and_unknown_prefixes(model):
    model.freeze_bn(layers=["bn1", "layer2.0.bn3"])
    assert model.frozen_bn == frozenset({"bn1", "layer2.0.bn3"})
    off = sorted(k for k, p in model.named_parameters() if not p.requires_grad)
    assert off == ["bn1.bias", "bn1.weight", "layer2.0.bn3.bias", "layer2.0.bn3.weight"]
    model.freeze_bn(layers=("layer1.0.bn1",), affine=False)                     # adds to the set
    assert model.frozen_bn == frozenset({"bn1", "layer2.0.bn3", "layer1.0.bn1"})
    assert model.get_tensor("layer1.0.bn1.weight").requires_grad
    for bad in (["layer4.0.bn1"], ["conv1"], ["bn1.weight"], ["layer2.0"]):
        with pytest.raises(ValueError):
            model.freeze_bn(layers=bad)
    assert model.frozen_bn == frozenset({"bn1", "layer2.0.bn3", "layer1.0.bn1"})   # a refused call changes nothing
    model.freeze_bn(False, layers=["bn1"])
    assert model.frozen_bn == frozenset({"layer2.0.bn3", "layer1.0.bn1"})
    assert model.get_tensor("bn1.weight").requires_grad and not model.get_tensor("layer2.0.bn3.weight").requires_grad


def test_unfreeze_restores_only_what_freeze_cleared(model):
    model.get_tensor("layer1.0.bn2.weight").requires_grad_(False)               # the user's own choice, made before freeze_bn
    model.freeze_bn()
    assert model.freeze_bn(False) is model
    assert model.frozen_bn == frozenset()
    off = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert off == ["layer1.0.bn2.weight"]


def test_train_and_eval_leave_the_frozen_set_alone(model):
    model.freeze_bn(layers=["bn1"], affine=False)
    for call in (model.train, model.eval, model.train):
        call()
        assert model.frozen_bn == frozenset({"bn1"})
    assert model.training
    eng = model._engine
    assert not eng.bn_batch_stats("bn1") and eng.bn_batch_stats("layer1.0.bn1")
    model.eval()
    assert not eng.bn_batch_stats("bn1") and not eng.bn_batch_stats("layer1.0.bn1")


def test_kg_bn_bwd_frozen_abi():
    """header prototype, ctypes table and the exports of BOTH libraries (bf16 rows / IEEE-half rows) agree"""
    from kg_instance_segmentation_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    m = re.search(r"\bint\s+kg_bn_bwd_frozen\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, "prototype missing from include/kgnet_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _lib._SIGS["kg_bn_bwd_frozen"]
    assert len(args) == len(sig) == 19
    for a, t in zip(args, sig):
        want = _lib.P if "*" in a else (_lib.c_float if a.startswith("float ") else _lib.c_int)
        assert t is want, (a, t)
    for path in (build.LIB, build.LIB_F16):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "kg_bn_bwd_frozen"), path
        lib.kg_last_error.restype = ctypes.c_char_p
        fn = lib.kg_bn_bwd_frozen
        fn.argtypes, fn.restype = sig, ctypes.c_int
        # argument validation happens on the host before any launch
        rc = fn(None, 0, None, 0, None, None, None, 1e-5, None, None, 0, None, 0, 1, 8, None, 0, None, None)
        assert rc != 0 and b"kg_bn_bwd_frozen" in lib.kg_last_error()
