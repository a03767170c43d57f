"""The contract of a module that fuses itself, the same for the three tiers of bnn_amd/dispatch.py — BlockFusion (a
residual block), OpFusion (a BATS cell operation), CellFusion (a whole BATS cell): a fused call is counted and its
executor cached; every condition that sends the call to the module's own forward declines exactly once; a refusal by
the executor is remembered until a parameter changes; copies carry a fresh state of the same class."""
import copy
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import models
from bnn_amd.inference import (BlockFusion, CellFusion, OpFusion, auto_block_forward, auto_cell_forward,
                               auto_op_forward, no_cell_fusion, per_layer_forward)
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import cellops_cases, cells_cases, gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, ref):
    """The project's layer bar."""
    a, ref = a.cpu().numpy(), ref.cpu().numpy()
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


def _load(model, state):
    model = bnn.prepare_binary_model(model, bnn.BConfig(
        activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
        weight_pre_process=XNORWeightBinarizer))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state(shapes).items()})
    return model.to(DEV).eval()


def _block():
    blk = _load(models.BasicBlock(64, 64), lambda shapes: gen.model_state(shapes, 1))
    return blk, (dev(gen.normal(gen.seed_of("tiers", "block"), (2, 64, 8, 8))),)


def _op():
    case = cellops_cases.CELL_CASES[0]
    return _load(case.build(models), case.state), (dev(case.input()),)


def _cell():
    case = cells_cases.CELL_CASES[0]
    return _load(case.build(models), case.state), tuple(dev(a) for a in case.inputs())


def _refuse_block(blk):
    act, blk.act1 = blk.act1, nn.Sigmoid()
    return lambda: setattr(blk, "act1", act)


def _refuse_op(op):
    op.op[1].padding_mode = "reflect"
    return lambda: setattr(op.op[1], "padding_mode", "zeros")


def _refuse_cell(cell):
    cell.use_shake_shake = True
    return lambda: setattr(cell, "use_shake_shake", False)


# name: (tier class, its key in module.__dict__, module and inputs, what the module's forward calls first, a change the
# executor refuses (returns its undo))
TIERS = {
    "block": (BlockFusion, "_bnn_auto_block", _block, auto_block_forward, _refuse_block),
    "op": (OpFusion, "_bnn_auto_op", _op, auto_op_forward, _refuse_op),
    "cell": (CellFusion, "_bnn_auto_cell", _cell, auto_cell_forward, _refuse_cell),
}


@pytest.mark.parametrize("tier", list(TIERS))
def test_tier_contract(tier, monkeypatch):
    cls, key, make, auto_forward, refuse = TIERS[tier]
    module, inputs = make()
    with torch.no_grad():
        # ---- a fused call
        y = module(*inputs)
        st = module.__dict__[key]
        assert type(st) is cls and st.calls == {"fused": 1, "declined": 0}
        eng = st.engine
        assert eng is not None and st.failed_sig is None

        # ---- declines: exactly one each, nothing fused
        def declines(fn, through_module):
            before = dict(st.calls)
            out = fn()
            assert st.calls == {"fused": before["fused"], "declined": before["declined"] + 1}
            if through_module:      # the module's own forward ran instead
                err = float((out - y).abs().max() / y.abs().max())
                print(f"{tier}: own forward vs fused, max |diff| / max |fused| = {err:.3g}")
                assert close(out, y)
            else:
                assert out is None

        declines(lambda: st.run(module, *(x[:0] for x in inputs)), False)            # an empty batch
        declines(lambda: st.run(module, *(x.half() for x in inputs)), False)         # not fp32
        module._is_replica = True
        declines(lambda: st.run(module, *inputs), False)
        del module._is_replica
        for name in ("BNN_AMD_AUTOFUSE", "BNN_AMD_STRICT_WEIGHTS"):
            monkeypatch.setenv(name, "0" if name == "BNN_AMD_AUTOFUSE" else "1")
            declines(lambda: module(*inputs), True)
            monkeypatch.delenv(name)
        with per_layer_forward():
            declines(lambda: module(*inputs), True)
        inner = next(m for m in module.modules() if isinstance(m, nn.Conv2d))
        hook = inner.register_forward_hook(lambda m, i, o: None)
        declines(lambda: module(*inputs), True)                                     # the hook must fire
        hook.remove()
        if tier == "cell":
            with no_cell_fusion():
                declines(lambda: module(*inputs), True)
        assert st.engine is eng and module.__dict__[key] is st
        assert torch.equal(module(*inputs), y) and st.engine is eng                 # still cached, same bits

        # ---- copies: a fresh state of the same class
        for twin in (copy.deepcopy(module), pickle.loads(pickle.dumps(module))):
            st2 = twin.__dict__[key]
            assert type(st2) is cls and st2 is not st and st2.engine is None
            assert st2.calls == {"fused": 0, "declined": 0}

        # ---- a refusal by the executor is remembered until a parameter changes
        module, inputs = make()
        undo = refuse(module)
        assert auto_forward(module, *inputs) is None and auto_forward(module, *inputs) is None
        st = module.__dict__[key]
        assert st.engine is None and st.failed_sig is not None
        assert st.calls == {"fused": 0, "declined": 2}
        undo()
        assert auto_forward(module, *inputs) is None                # same parameter signature: not tried again
        assert st.engine is None and st.calls == {"fused": 0, "declined": 3}
        next(module.parameters()).add_(0)                           # same values, a new version
        out = auto_forward(module, *inputs)
        assert out is not None and torch.equal(out, y)
        assert st.engine is not None and st.calls == {"fused": 1, "declined": 3}
