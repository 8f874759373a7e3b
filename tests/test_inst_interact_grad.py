"""The backward of the head's instance interaction without a GPU: the C ABI's declaration, the host restatement
(interact.inst_interact_host under torch's autograd) against the gradients the reference's own RCNNHead / RCNNHead_cond backpropagate
(tests/golden/inst_interact/grads.npz), the exact zeros of a dead unit, inst_interact on CPU tensors, what
loss_gradients(through="interact") refuses, and that the seeded cases of the GPU tests keep off the kinks."""
import os

import pytest
import torch

from conftest import ROOT

import _inst_interact_cases as IC

from diffusionvid_amd import _lib
from diffusionvid_amd.modeling.roi_heads.box_head import interact as I


def test_abi_carries_the_interaction_entry_points():
    """fails before the interaction's backward exists: the header, _lib.SIGNATURES and the library carry the three symbols, dvid_version() >= 15"""
    with open(os.path.join(ROOT, "include", "dvid_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("dvid_inst_interact_backward", "dvid_inst_interact_backward_scratch_bytes", "dvid_rcnn_head_levels_keep2"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = header.split(" %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1])
    assert lib.dvid_version() >= 15
    doc = header.split("dvid_inst_interact_backward (dvid_version >= 15)")[1].split("*/")[0]
    at = [doc.index(" %s" % k) for k in I.PARAM_NAMES[::2]]          # the documented order of the pointer table is interact.PARAM_NAMES
    assert at == sorted(at) and len(I.PARAM_NAMES) == 12 and all(k.endswith(".weight") for k in I.PARAM_NAMES[::2])
    for words in ("ReLU passes nothing at a pre-activation of exactly 0", "no atomics", "DVID_INST_BWD_ROW_SLAB"):
        assert words in doc, words
    slab = int(header.split("#define DVID_INST_BWD_ROW_SLAB ")[1].split()[0])
    assert slab % 256 == 0 and slab <= 1024
    # the scratch query needs no device.  params and d_params exist for one slab: past it only the terms per row grow
    q = lib.dvid_inst_interact_backward_scratch_bytes
    assert 0 < q(1) < q(slab) and q(0) == -1 and q(1048577) == -1
    per_row = (q(4 * slab) - q(2 * slab)) / (2 * slab)
    assert 2 * 49 * 256 * 4 <= per_row < 2 * 49 * 256 * 4 + 16 * 1024 and q(slab) - q(slab // 2) > (slab // 2) * 2 * 32768 * 4


def test_the_entry_point_refuses_before_any_launch():
    """sizes first, with the numbers in the message; then null pointers (no device is touched: every pointer here is null)"""
    lib = _lib.load()

    def refused(rows=5, hidden=256, dd=64, pooler=7, n_params=12):
        rc = lib.dvid_inst_interact_backward(None, None, rows, hidden, dd, pooler, None, n_params, *([None] * 6), 0, None)
        return rc, lib.dvid_last_error().decode()

    for kw, code, words in (({"hidden": 128}, 3, "hidden size 128"), ({"dd": 32}, 3, "dim_dynamic 32"), ({"pooler": 14}, 3, "14 x 14 pooler"),
                            ({"rows": 0}, 1, "0 rows"), ({"rows": 1048577}, 3, "1048577 rows"), ({"n_params": 14}, 1, "14 parameter pointers"),
                            ({}, 1, "null pointer")):
        rc, msg = refused(**kw)
        assert rc == code and words in msg and msg.startswith("instance interaction backward:"), (kw, rc, msg)


def test_fixture_holds_every_case():
    fx = IC.fixture()
    assert tuple(sorted(fx)) == IC.NAMES
    for name, c in fx.items():
        assert c["in"]["p"].shape == (14, 16) and c["in"]["roi"].shape == (14, 49, 16) and c["cot"].shape == (14, 16)
        assert sorted(c["sd"]) == sorted(I.PARAM_NAMES) and c["sd"]["inst_interact.dynamic_layer.weight"].shape == (2 * 16 * 4, 16)
        assert sorted(c["grad"]) == sorted(["p", "roi"] + list(c["sd"])) and sorted(c["dev32"]) == sorted(list(c["grad"]) + ["y"])
        assert all(v.dtype == "float32" for v in list(c["grad"].values()) + list(c["out"].values()))
    sd = fx["plain_dead_unit"]["sd"]
    assert sd["inst_interact.norm2.weight"][IC.DEAD] == 0 and sd["inst_interact.norm2.bias"][IC.DEAD] == 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "inst_interact", "grads.npz")) < 1 << 20


def _host(case, dtype):
    return IC.host_run(I, case["in"]["p"], case["in"]["roi"], case["sd"], case["cot"], dtype)


@pytest.mark.parametrize("name", IC.NAMES)
def test_inst_interact_host_meets_the_reference(name):
    """float64: the stored truth is the reference's float64 run rounded to float32, so the float64 result is rounded the same way before the
    1e-10 comparison.  fp32: within the bound of the reference's own fp32 run, per tensor, and the run reproduces that yardstick within a
    factor of 2: it deviates by no more than twice what the reference's fp32 run does (floored at 2^-24; the two differ in summation
    order only, and a run that happens to land closer to the truth -- seen: 1.3e-07 against 3.9e-07 -- is no miss)."""
    case = IC.fixture()[name]
    y, grads = _host(case, torch.float64)
    assert sorted(grads) == sorted(case["grad"])
    for k, v in [("y", y)] + list(grads.items()):
        assert v.dtype == torch.float64
        assert IC.deviation(v.float(), case["out" if k == "y" else "grad"][k]) <= 1e-10, k
    y, grads = _host(case, torch.float32)
    for k, v in [("y", y)] + list(grads.items()):
        dev, yard = IC.deviation(v, case["out" if k == "y" else "grad"][k]), float(case["dev32"][k])
        assert v.dtype == torch.float32 and dev <= IC.bound(yard), (k, dev, yard)
        assert dev <= 2 * max(yard, 2.0 ** -24), (k, dev, yard)


def test_a_dead_unit_gets_exact_zeros_where_the_reference_does():
    case = IC.fixture()["plain_dead_unit"]
    for dtype in (torch.float64, torch.float32):
        _, grads = _host(case, dtype)
        for k, want in case["grad"].items():
            zero = torch.from_numpy(want) == 0
            assert bool((grads[k][zero] == 0).all()), k
        assert grads["inst_interact.norm2.weight"][IC.DEAD] == 0 and grads["inst_interact.norm2.bias"][IC.DEAD] == 0
        assert not bool(grads["inst_interact.out_layer.weight"].reshape(16, 49, 16)[:, :, IC.DEAD].any())
        assert bool(grads["inst_interact.out_layer.weight"].reshape(16, 49, 16)[:, :, IC.DEAD - 1].any())


def test_inst_interact_on_cpu_tensors_is_autograd_on_the_host_path():
    case = IC.fixture()["cond"]
    _, want = _host(case, torch.float32)
    leaf = lambda a: torch.from_numpy(a).clone().requires_grad_(True)
    p, roi, w = leaf(case["in"]["p"]), leaf(case["in"]["roi"]), {k: leaf(v) for k, v in case["sd"].items()}
    (torch.from_numpy(case["cot"]) * I.inst_interact(p, roi, w)).sum().backward()
    got = {"p": p.grad, "roi": roi.grad, **{k: v.grad for k, v in w.items()}}
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_what_loss_gradients_through_interact_refuses():
    """each by name, before anything is built or launched; the unknown-value message lists all three values"""
    from test_head_tail_grad import _model
    from diffusionvid_amd.structures.bounding_box import BoxList
    target = BoxList(torch.tensor([[4.0, 4.0, 20.0, 20.0]]), (32, 32), mode="xyxy")
    target.add_field("labels", torch.ones(1, dtype=torch.int64))
    batch = ([torch.zeros(3, 32, 32)], [target])
    model = _model(["DTYPE", "float32"])
    assert model.objective.THROUGH == ("outputs", "tail", "interact")
    with pytest.raises(ValueError, match=r"loss_gradients: through='heads'.*'outputs', 'tail', 'interact'"):
        model.loss_gradients(*batch, through="heads")
    assert model._engine is None
    model = _model(["DTYPE", "float16"])
    with pytest.raises(NotImplementedError, match=r"loss_gradients: through='interact' needs DTYPE float32.*float16"):
        model.loss_gradients(*batch, through="interact", roi_gradients=True)
    assert model._engine is None
    model = _model(["DTYPE", "float32", "MODEL.DiffusionDet.DROPOUT", 0.1])
    with pytest.raises(NotImplementedError, match=r"loss_gradients: MODEL\.DiffusionDet\.DROPOUT is 0\.1"):
        model.loss_gradients(*batch, through="interact")
    assert model._engine is None


@pytest.mark.parametrize("seed,R", ((11, 1), (12, 111)))
def test_the_settled_cases_are_settled(seed, R):
    """no ReLU pre-activation within 0.9 MARGIN of 0 in the float64 forward, and only the three biases were moved, by less than 400 MARGIN"""
    c = IC.make_case(seed, R)
    for a in IC.pre_activations(c["p"], c["roi"], c["params"]):
        assert float(a.abs().min()) >= 0.9 * IC.MARGIN
    raw = IC.link_params(seed % 7)
    for k in I.PARAM_NAMES:
        moved = k in ("inst_interact.norm1.bias", "inst_interact.norm2.bias", "inst_interact.norm3.bias")
        assert moved or torch.equal(raw[k], c["params"][k]), k
        assert float((raw[k] - c["params"][k]).abs().max()) < 400 * IC.MARGIN
