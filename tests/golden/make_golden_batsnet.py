#!/usr/bin/env python3
"""Generate tests/golden/batsnet.npz by running the REFERENCE implementation of BATSNetworkCIFAR with a real-valued stem
and classifier (tests/golden/batsnet_cases.py).

Runs only where the reference package is importable; the test-suite and the GPU box use the committed ``batsnet.npz``.
Generated exactly as make_golden_cells.py does it: inputs and state from gen.py seeds, the salt searched until fp32 and
fp64 agree on every sign() and the sign margin clears MARGIN_FACTOR x e_ref; the reference's logits, the state_dict key
list, the salt, the margin and e_ref are stored.  The salt printed must be the one committed in batsnet_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_batsnet.py [--find]
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("BNN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)

import torch  # noqa: E402

import bnn  # the reference package  # noqa: E402
from bnn import ops  # noqa: E402
from bnn.models import bats  # noqa: E402

from tests.golden.batsnet_cases import BATSNET_CASE, binarise_real_ends, sign_inputs  # noqa: E402
from tests.golden.cells_cases import MARGIN_FACTOR, sign_margin  # noqa: E402

assert os.path.realpath(bnn.__file__).startswith(os.path.realpath(REFERENCE)), bnn.__file__
torch.set_num_threads(8)
MAX_SALT = 64


def try_salt(case, salt):
    """(out, keys, margin, e_ref) of the reference at this salt, or None when a sign() sits too close to 0."""
    model = binarise_real_ends(bnn, ops, case.build(bats))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes, salt).items()})
    model.eval()
    x32 = tuple(torch.from_numpy(a) for a in case.inputs(salt))
    model64 = copy.deepcopy(model).double()
    with torch.no_grad():
        out, seen32 = sign_inputs(model, case, x32)
        _, seen64 = sign_inputs(model64, case, tuple(a.double() for a in x32))
    assert len(seen32) == len(seen64) > 0
    same = all(torch.equal(torch.sign(a).double(), torch.sign(b)) for a, b in zip(seen32, seen64))
    e_ref = max(float((a.double() - b).abs().max()) for a, b in zip(seen32, seen64))
    margin = sign_margin(seen32)
    if not same or margin < MARGIN_FACTOR * e_ref:
        print(f"   {case.name} salt {salt}: margin {margin:.3g} < {MARGIN_FACTOR:g} x e_ref {e_ref:.3g}"
              f"{'' if same else ' (fp32 and fp64 disagree on a sign)'}: next salt")
        return None
    return out.numpy().copy(), list(shapes), margin, e_ref


def main():
    find = "--find" in sys.argv[1:]
    case = BATSNET_CASE
    for salt in range(MAX_SALT):
        got = try_salt(case, salt)
        if got is not None:
            break
    else:
        raise SystemExit(f"{case.name}: no salt below {MAX_SALT} clears the margin")
    out, keys, margin, e_ref = got
    assert find or salt == case.salt, \
        f"{case.name}: the first salt that clears the margin is {salt}; commit it in batsnet_cases.py"
    print(f"batsnet {case.name} salt={salt} out{out.shape} |max|={np.abs(out).max():.4f} margin={margin:.3g} "
          f"e_ref={e_ref:.3g} keys={len(keys)}")
    if find:
        return
    np.savez_compressed(os.path.join(HERE, "batsnet.npz"), **{
        case.name + "/out": out, case.name + "/keys": np.array(keys), case.name + "/margin": np.float64(margin),
        case.name + "/e_ref": np.float64(e_ref), case.name + "/salt": np.int64(salt)})


if __name__ == "__main__":
    main()
