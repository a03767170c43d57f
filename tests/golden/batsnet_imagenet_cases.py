"""Golden case of the two real-valued stems of a BATS ImageNet network (used by make_golden_batsnet_imagenet.py and the
tests): the reference's BATSNetworkImageNet(*IMAGENET_ARGS, MIXED, GROUPS) (bnn/models/bats.py:154-206), binarised with
prepare_binary_model except REAL_LAYERS, which keep an all-Identity recipe the way the reference's examples keep first
and last layers real (custom_config_layers_name={...: BConfig()}).  Only the stems run: no sign() is involved, so the case
needs no salt, and a small image does (the stems alone do not need 224 x 224).  State and input come from gen.py seeds."""
from __future__ import annotations

from . import gen
from .cells_cases import GROUPS, IMAGENET_ARGS, genotype

REAL_LAYERS = ("stem0.0", "stem0.3", "stem1.1", "classifier")
NAME = "imagenet_net_real_stems"
XSHAPE = (2, 3, 20, 18)
SEED = gen.seed_of("cells", NAME, 0)


def build(ns):
    """The float network from the classes of ``ns`` (the reference's bnn.models.bats, or bnn_amd.models)."""
    net = ns.BATSNetworkImageNet(*IMAGENET_ARGS, genotype(ns, "MIXED"), GROUPS)
    net.drop_path_prob = 0.0
    return net


def binarise_real_stems(bnn, ops, model):
    """``prepare_binary_model`` with the usual recipe and REAL_LAYERS real-valued; ``bnn`` / ``ops`` are the package and
    its ops module (the reference's, or bnn_amd's)."""
    cfg = bnn.BConfig(activation_pre_process=ops.BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=ops.XNORWeightBinarizer)
    return bnn.prepare_binary_model(model, cfg, custom_config_layers_name={n: bnn.BConfig() for n in REAL_LAYERS})


def inputs():
    return gen.activation("normal", SEED, XSHAPE)


def state(shapes: dict) -> dict:
    return gen.model_state(shapes, SEED)


def run_stems(model, x):
    """``(s0 before stem1 ran, s0 after it, s1)``: stem1 starts with an in-place ReLU, so the tensor stem0 returned is
    rectified by the time the cells read it."""
    s0 = model.stem0(x)
    raw = s0.detach().clone()
    s1 = model.stem1(s0)
    return raw, s0, s1
