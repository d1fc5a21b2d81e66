"""The dispatch of csrc/ldn_conv_image.hip (dispatch_mode :1738-1754, launch_shape :1680-1700, launch_k :1647-1677) restated in Python:
which kernel, tile shape and weight-staging mode a launch of ldn_conv_packed or ldn_conv_image runs.  tests/test_hip_packed.py and
tests/test_hip_conv_image.py prove from it, on the CPU, that their case tables run every instantiation a launch can reach.  No CUDA here."""
from __future__ import annotations


def expected_variant(packed, rows_per_image, cin, cout, taps, has_k, has_n, kgran, shift_classes, residual, scale, math, out_split=False):
    """(kernel, MS, NS, BMODE) a conv launch runs, transcribed from csrc/ldn_conv_image.hip.  rows_per_image: m_cap of a packed launch,
    Ho * Wo of an image launch (:1683); taps: 1 or 9 (:1739); has_k / has_n: input / output channel list; math: "fp32" | "bf16x3";
    out_split: out_format 1 of ldn_conv_image (only k_conv_bf3's epilogue writes it)."""
    bf3 = math == "bf16x3"
    hw = rows_per_image
    # dispatch_mode, :1745-1748: the streaming kernel (ST_BM = ST_BN = 128, :1246; LDN_STREAM_ROWS at its default 512, :1707)
    if (bf3 and taps == 1 and not has_n and shift_classes == 1 and cout % 128 == 0 and cout >= 2 * 128
            and not (residual and scale) and cin <= 1024 and hw >= 96 and not out_split):
        return ("k_conv1x1_stream", None, None, "B_KN4" if has_k else "B_NK")
    # :1749-1753: how the weights are staged
    if not has_k:
        bmode = "B_NK"
    else:
        g = kgran if has_n else 4
        bmode = "B_KN4" if g % 4 == 0 else ("B_KN2" if g % 2 == 0 else "B_KN1")
    # launch_shape, :1680-1700
    nsubs = -(-cout // 32)
    if nsubs <= 4:
        per = nsubs
    elif hw <= 128:
        per = min(nsubs, 10)
    elif hw <= 256 and has_n:
        per = min(nsubs, 6)
    else:
        per = 4
    if per <= 2:
        ms, ns = 6, 2
    elif per <= 4:
        ms, ns = 4, 4
    elif per <= 6:
        ms, ns = 8, 6
    else:
        ms, ns = 4, 10
    # launch_k, :1648-1661 (bf16x3) / :1662-1676 (fp32)
    if bf3:
        if (ms, ns) == (4, 10) and -(-hw // 32) <= 2:      # :1652-1654, the 2 x 10 special case
            ms = 2
        return ("k_conv_bf3", ms, ns, bmode)
    return ("k_conv_image", ms, ns, bmode)


def expected_wave_rows(variant, residual):
    """WM of k_conv_bf3 (:1655-1660): the 4 x 4 tile runs a 4 x 1 wave grid without a residual and 2 x 2 with one."""
    kernel, ms, ns, _ = variant
    if kernel != "k_conv_bf3":
        return None
    if (ms, ns) == (4, 4) and not residual:
        return 4
    return 4 if ms >= 8 else 2
