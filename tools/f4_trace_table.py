#!/usr/bin/env python3
"""The per-launch table of profiles/mfma_f4_kernel_roofline.md from the four traces tools/f4_trace.sh leaves in
build/f4trace/ or $F4_TRACE_DIR (zero1, all1, zero2, all2): last whole forward of each trace, stem to stem.  Prints the table, the
sums and, per matrix-core launch, whether both `=all` values lie below both `=0` values by more than the launch's gap
(the admission rule of fastpath.MFMA_F4_SHAPES)."""
import csv, glob, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.environ.get("F4_TRACE_DIR") or os.path.join(ROOT, "build", "f4trace")
N = 256
TAGS = ("zero1", "zero2", "all1", "all2")

# the 19 launches of bnn_amd/inference.py for resnet18: (label, C, O, Hout, shortcut channels or 0, on the matrix cores)
L = [("stem", 3, 64, 56, 0, False)]
L += [("layer1.%d.conv%d" % (b, c), 64, 64, 56, 0, False) for b in (0, 1) for c in (1, 2)]
for li, (ci, co, ho) in enumerate(((64, 128, 28), (128, 256, 14), (256, 512, 7)), start=2):
    L += [("layer%d.0.conv1 (stride 2)" % li, ci, co, ho, 0, ci >= 128),
          ("layer%d.0.conv2 + folded shortcut" % li, co, co, ho, ci, True),
          ("layer%d.1.conv1" % li, co, co, ho, 0, True), ("layer%d.1.conv2" % li, co, co, ho, 0, True)]
L += [("avgpool (head 1/2)", 512, 512, 1, 0, False), ("fc (head 2/2)", 512, 1000, 1, 0, False)]


def forward(tag):
    f = glob.glob(os.path.join(D, tag, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    st = [i for i, r in enumerate(rows) if "stem_rows" in r["Kernel_Name"]]
    step = rows[st[-2]:st[-1]]
    assert len(step) == len(L), (tag, len(step))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in step]
    span = (int(rows[st[-1]]["Start_Timestamp"]) - int(step[0]["Start_Timestamp"])) / 1e3
    names = [r["Kernel_Name"] for r in step]
    return us, span, names


fw = {t: forward(t) for t in TAGS}
out = ["| launch | `=0` us (1) | `=0` us (2) | `=all` us (1) | `=all` us (2) | gap | all − 0 (means) | matrix floor us (FP4) | "
       "HBM floor us | max(floor) / `=all` | admitted |", "|---|---|---|---|---|---|---|---|---|---|---|"]
admitted = []
for i, (label, C, O, H, sc, cores) in enumerate(L):
    z1, z2, a1, a2 = (fw[t][0][i] for t in TAGS)
    gap = max(abs(z1 - z2), abs(a1 - a2))
    diff = (a1 + a2) / 2 - (z1 + z2) / 2
    f4 = cores and C % 128 == 0
    extra = ["", "", "", ""]
    if f4:
        macs = N * H * H * O * (9 * C + sc)
        # input planes (P only: non-negative activations) + fp32 output + output planes; the FP4 pack; the fp32 residual
        # where there is one (conv2 without a folded shortcut)
        stride = 2 if "stride 2" in label else 1
        hin = H * stride
        byts = N * hin * hin * C / 8 + N * H * H * O / 8 + 9 * C * O / 2
        if "conv2" in label or "conv1" not in label:
            byts += N * H * H * O * 4 * (1 if sc or H > 7 else 2)   # (layer2 / 3 .1.conv2 write planes only)
        if sc:
            byts += N * (2 * H) * (2 * H) * sc / 8
        mf, hf = macs / 5e15 * 1e6, byts / 8e12 * 1e6
        ok = max(a1, a2) < min(z1, z2) - gap
        extra = ["%.1f" % mf, "%.1f" % hf, "%.2f" % (max(mf, hf) / ((a1 + a2) / 2)), "yes" if ok else "no"]
        if ok:
            admitted.append((label, C, O, H * stride, stride, sc, (z1 + z2) / 2, (a1 + a2) / 2))
    name = "**%s**" % label if f4 else label
    out.append("| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %+.1f | %s |" % (name, z1, z2, a1, a2, gap, diff, " | ".join(extra)))
print("\n".join(out))
print()
for kind, (x, y) in (("=0", ("zero1", "zero2")), ("=all", ("all1", "all2"))):
    print("`%s`: sums %.1f / %.1f us; stem-to-stem %.1f / %.1f us; %d launches." % (
        kind, sum(fw[x][0]), sum(fw[y][0]), fw[x][1], fw[y][1], len(L)))
cores = [i for i, l in enumerate(L) if l[5] and l[1] % 128 == 0]
print("matrix-core launches with C %% 128 == 0: =0 %.1f / %.1f us, =all %.1f / %.1f us; summed gaps %.1f us" % (
    *(sum(fw[t][0][i] for i in cores) for t in TAGS),
    sum(max(abs(fw["zero1"][0][i] - fw["zero2"][0][i]), abs(fw["all1"][0][i] - fw["all2"][0][i])) for i in range(len(L)))))
print()
print("MFMA_F4_SHAPES candidates (dense key (C, O, H, stride, False), fold key (C, O, H, sc_C)):")
for label, C, O, H, stride, sc, z, a in admitted:
    key = (C, O, H, sc) if sc else (C, O, H, stride, False)
    print("    %s: (%.1f, %.1f),   # %s" % (key, z, a, label))
if "--kernels" in sys.argv:
    for t in ("zero1", "all1"):
        print(t, *[n.split("(")[0][-60:] for n in fw[t][2]], sep="\n  ")
