"""Golden cases of whole BATS cells and networks (used by make_golden_cells.py and the tests): the reference's Cell /
BATSNetworkCIFAR / BATSNetworkImageNet (bnn/models/bats.py), binarised with prepare_binary_model, eval mode,
drop_prob = 0.

The reference publishes no genotype, so two are defined here: MIXED has every primitive next to a convolution, ALLCONV
has nodes made of two convolutions, a `none`, and a state read by four operations.

A cell binarises its own intermediate sums, so a value within rounding distance of 0 in front of a sign() lets two
correct implementations differ.  Every case therefore carries a SALT, chosen by the generator as the first one for
which the smallest |input| of any binary layer is at least MARGIN_FACTOR times the reference's own fp32-vs-fp64
difference over those inputs: two fp32 implementations can each be that far from the exact value, the factor 4 is twice
that worst case.  "Change the seed, not the bound."
"""
from __future__ import annotations

from dataclasses import dataclass

from . import gen

MIXED = dict(
    normal=[("sep_conv_3x3", 0), ("dil_conv_3x3", 1), ("skip_connect", 0), ("sep_conv_5x5", 2),
            ("avg_pool_3x3", 1), ("dil_conv_5x5", 3), ("max_pool_3x3", 2), ("skip_connect", 3)],
    normal_concat=[2, 3, 4, 5],
    reduce=[("sep_conv_3x3", 0), ("skip_connect", 1), ("max_pool_3x3", 0), ("dil_conv_3x3", 1),
            ("skip_connect", 2), ("sep_conv_5x5", 3), ("avg_pool_3x3", 1), ("dil_conv_5x5", 2)],
    reduce_concat=[2, 3, 4, 5])
ALLCONV = dict(
    normal=[("sep_conv_3x3", 0), ("sep_conv_3x3", 1), ("dil_conv_3x3", 0), ("dil_conv_5x5", 1),
            ("sep_conv_5x5", 1), ("sep_conv_3x3", 2), ("none", 0), ("dil_conv_3x3", 1)],
    normal_concat=[3, 4, 5],
    reduce=[("sep_conv_3x3", 0), ("sep_conv_3x3", 1)] * 4,
    reduce_concat=[2, 3, 4, 5])
GENOTYPES = {"MIXED": MIXED, "ALLCONV": ALLCONV}
GROUPS = 12
N = 2
MARGIN_FACTOR = 4.0


def genotype(ns, name: str):
    return ns.Genotype(**GENOTYPES[name])


@dataclass(frozen=True)
class CellCase:
    name: str
    genotype: str
    args: tuple                # (C_prev_prev, C_prev, C, reduction, reduction_prev)
    hw0: tuple                 # H, W of s0
    hw1: tuple                 # H, W of s1
    salt: int                  # chosen by make_golden_cells.py (first salt that clears the sign margin)

    def build(self, ns):
        """The float cell from the classes of ``ns`` (the reference's bnn.models.bats, or bnn_amd.models)."""
        return ns.Cell(genotype(ns, self.genotype), *self.args, groups=GROUPS)

    def seed(self, salt=None) -> int:
        return gen.seed_of("cells", self.name, self.salt if salt is None else salt)

    def inputs(self, salt=None):
        s = self.seed(salt)
        return (gen.activation("normal", s, (N, self.args[0]) + self.hw0),
                gen.activation("normal", s + 1, (N, self.args[1]) + self.hw1))

    def state(self, shapes: dict, salt=None) -> dict:
        return gen.model_state(shapes, self.seed(salt))

    def run(self, model, inputs):
        return model(inputs[0], inputs[1], 0.0)


@dataclass(frozen=True)
class NetCase:
    name: str
    genotype: str
    args: tuple                # (C, num_classes, layers, auxiliary)
    xshape: tuple
    salt: int

    def build(self, ns):
        net = ns.BATSNetworkCIFAR(*self.args, genotype(ns, self.genotype), GROUPS)
        net.drop_path_prob = 0.0
        return net

    def seed(self, salt=None) -> int:
        return gen.seed_of("cells", self.name, self.salt if salt is None else salt)

    def inputs(self, salt=None):
        return (gen.activation("normal", self.seed(salt), self.xshape),)

    def state(self, shapes: dict, salt=None) -> dict:
        return gen.model_state(shapes, self.seed(salt))

    def run(self, model, inputs):
        return model(inputs[0])[0]


CELL_CASES = [
    CellCase("normal", "MIXED", (72, 96, 48, False, False), (8, 8), (8, 8), salt=0),
    CellCase("reduce", "MIXED", (96, 96, 48, True, False), (8, 8), (8, 8), salt=1),
    CellCase("after_reduce", "MIXED", (48, 96, 48, False, True), (16, 16), (8, 8), salt=1),
    CellCase("allconv_none", "ALLCONV", (96, 96, 96, False, False), (7, 9), (7, 9), salt=5),
]
NET_CASE = NetCase("cifar_net", "MIXED", (24, 10, 3, False), (N, 3, 16, 16), salt=0)
ALL_CASES = CELL_CASES + [NET_CASE]
IMAGENET_ARGS = (60, 10, 3, False)         # BATSNetworkImageNet(*IMAGENET_ARGS, MIXED, GROUPS): state_dict keys only


def binary_inputs(model, case, inputs):
    """``(output, [input of every binary layer, in call order])`` of one forward of ``model`` (torch tensors in)."""
    seen, hooks = [], []
    for m in model.modules():
        if hasattr(m, "activation_pre_process"):
            hooks.append(m.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].detach().clone())))
    try:
        out = case.run(model, inputs)
    finally:
        for h in hooks:
            h.remove()
    return out, seen


def sign_margin(seen) -> float:
    """min |input| over the recorded inputs of the binary layers."""
    return min(float(t.abs().min()) for t in seen)
