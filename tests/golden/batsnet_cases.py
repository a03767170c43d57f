"""Golden case of a whole BATS network with a REAL-valued stem and classifier (used by make_golden_batsnet.py and the
tests): the reference's BATSNetworkCIFAR (bnn/models/bats.py) at the size of cells_cases.NET_CASE, binarised with
prepare_binary_model except ``stem.0`` and ``classifier``, which keep an all-Identity recipe the way the reference's
examples keep first and last layers real (custom_config_layers_name={...: BConfig()}).  Inputs, parameters, the salt
search and the sign margin are those of cells_cases.py."""
from __future__ import annotations

from .cells_cases import NetCase

REAL_LAYERS = ("stem.0", "classifier")
BATSNET_CASE = NetCase("cifar_net_real_stem", "MIXED", (24, 10, 3, False), (2, 3, 16, 16), salt=27)


def binarise_real_ends(bnn, ops, model):
    """``prepare_binary_model`` with the usual recipe and REAL_LAYERS real-valued; ``bnn`` / ``ops`` are the package and
    its ops module (the reference's, or bnn_amd's)."""
    cfg = bnn.BConfig(activation_pre_process=ops.BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=ops.XNORWeightBinarizer)
    return bnn.prepare_binary_model(model, cfg, custom_config_layers_name={n: bnn.BConfig() for n in REAL_LAYERS})


def sign_inputs(model, case, inputs):
    """``cells_cases.binary_inputs`` over the layers that do take a sign(): ``(output, [their inputs, in call order])``.
    The real-valued stem convolution and classifier are binary-class layers with an Identity recipe; what they read (the
    image, the pooled features) is in front of no sign() and stays out of the margin."""
    seen, hooks = [], []
    for m in model.modules():
        if hasattr(m, "activation_pre_process") and type(m.activation_pre_process).__name__ != "Identity":
            hooks.append(m.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].detach().clone())))
    try:
        out = case.run(model, inputs)
    finally:
        for h in hooks:
            h.remove()
    return out, seen
