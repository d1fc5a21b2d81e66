"""Writes tests/golden/conv_plan_pins.txt: the plan conv_plan() (laudnet_amd/csrc/ldn_conv_plan.h) makes for every ldn_conv_image /
ldn_conv_packed shape the shipped models issue at the bench's batch size (256), from the models' layer tables.  No GPU.

    python tests/golden/make_conv_plan_pins.py        (after a deliberate tuning change; the diff of the pin file is part of that change)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import conv_plan as P  # noqa: E402

B = 256
MATHS = ("fp32", "bf16x3")


def launch(packed, rows, taps, cin, cout, has_k=False, has_n=False, kgran=1, residual=False, scale=True, out_split=False, images=B):
    return dict(packed=packed, B=images, rows_per_image=rows, taps=taps, cin=cin, cout=cout, has_k=has_k, has_n=has_n, kgran=kgran,
                shift_classes=16 if taps == 9 else 1, residual=residual, scale=scale, out_split=out_split)


def resnet_sections():
    """ResNet-50 and -101 differ in the number of blocks per stage, not in their shapes: per stage the first block (projection shortcut, the
    stride in the 3x3) and the others.  Channel granularity 2 (the bench's 2-2-2-2)."""
    gran, hi, cin = 2, 56, 64
    for stage, (w, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), 1):
        for first in (True, False):
            s = stride if first else 1
            ho = hi // s
            rin, rout, cout = hi * hi, ho * ho, 4 * w
            tag = f"ResNet-50/101 stage {stage} {'first block' if first else 'other blocks'} ({cin} -> {w} -> {cout}, {hi}x{hi} -> {ho}x{ho})"
            chan = [launch(False, rin, 1, cin, w, has_n=True, kgran=gran), launch(False, rin, 1, cin, w, has_n=True, kgran=gran, out_split=True),
                    launch(False, rout, 9, w, w, has_k=True, has_n=True, kgran=gran),
                    launch(False, rout, 1, w, cout, has_k=True, kgran=gran, residual=True, scale=False)]
            if first:
                chan.append(launch(False, rout, 1, cin, cout))
            yield tag + ", channel mode: conv1 (fp32 rows / pre-split), conv2, conv3" + (", projection" if first else ""), chan
            yield tag + ", channel mode executed densely on packed rows: conv1, conv2", [
                launch(True, B * rin, 1, cin, w, images=1), launch(True, B * rout, 9, w, w, images=1)]
            yield tag + ", both mode: conv1, conv2, conv3", [
                launch(True, rin, 1, cin, w, has_n=True), launch(True, rout, 9, w, w, has_k=True, has_n=True, kgran=gran),
                launch(True, rout, 1, w, cout, has_k=True, kgran=gran, residual=True, scale=False)]
            hi, cin = ho, cout


def regnet_sections():
    """The LAD-RegNetY family: per stage the first block (stride 2, projection) and the others.  conv a with an output list, conv c with an
    input list, a residual and its BN scale -- on whole images (channel mode) and on packed rows (layer-skip with channel masks)."""
    from laudnet_amd.laud_regnet import _Y, BlockParams
    for name, cfg in _Y.items():
        params = BlockParams.from_init_params(se_ratio=0.25, **cfg)
        hi, cin = 112, 32
        for stage, (w, stride, depth, _gw, mult) in enumerate(params._get_expanded_params(), 1):
            wb = int(round(w * mult))
            for first in (True, False)[:2 if depth > 1 else 1]:
                s = stride if first else 1
                ho = (hi - 1) // s + 1
                rin, rout = hi * hi, ho * ho
                ls = [launch(False, rin, 1, cin, wb, has_n=True), launch(False, rout, 1, wb, w, has_k=True, residual=True),
                      launch(True, rout, 1, wb, w, has_k=True, residual=True)]
                if first:
                    ls.append(launch(False, rout, 1, cin, w))
                yield (f"LAD-RegNetY-{name} stage {stage} {'first block' if first else 'other blocks'} ({cin} -> {wb} -> {w}, {hi}x{hi} -> {ho}x{ho}): "
                       "conv a, conv c, conv c on packed rows" + (", projection" if first else "")), ls
                hi, cin = ho, w


def main():
    out = ["# The plan conv_plan() (laudnet_amd/csrc/ldn_conv_plan.h) makes for the ldn_conv_image / ldn_conv_packed shapes the shipped models issue",
           "# at batch 256, in both arithmetic modes, LDN_STREAM_ROWS at its default.  tests/test_conv_plan.py fails on any change: a tuning change",
           "# edits this file with it (tests/golden/make_conv_plan_pins.py writes it).  The spatial and layer modes of the ResNets issue",
           "# ldn_conv_rows launches only (tests/golden/dense_plan_pins.txt).",
           "# packed|image math B rows taps cin cout has_k has_n kgran shift_classes residual scale out_split stream_rows"
           " kernel bn ntn bm mtn grid lds_bytes"]
    seen = set()
    for sections in (resnet_sections(), regnet_sections()):
        for tag, launches in sections:
            lines = [P.shape_line(math=m, **kw) for kw in launches for m in MATHS if not (kw["out_split"] and m == "fp32")]
            lines = [ln for ln in lines if ln not in seen and not seen.add(ln)]
            if lines:
                out.append("# " + tag)
                out.extend(P.run(lines))
    with open(os.path.join(HERE, "conv_plan_pins.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"{sum(not ln.startswith('#') for ln in out)} pins")


if __name__ == "__main__":
    main()
