"""Mutant nets for tests/test_parity_bars.py: a shipped .bin with ONE array rewritten in place, the shapes untouched -- every
kernel runs on it as it runs on the shipped net, and its output is wrong by a small, known amount.  What the fp32-oracle bars
are asked: do they tell such a net from the shipped one?

    tail_bias   every bias of the last convolution + amount / 255: a DC offset of `amount` levels in the output (what a biased
                rounding in a tail kernel would leave); no row or column stands out, so the structure statistic is blind to it
    slope       the PReLU slopes of one middle trunk layer x (1 + amount): an error that follows the content

The byte offsets come from walking the .param with the oracle side's parser (oracle/generic_oracle.py parse_param /
conv_shapes), and write_mutant_bin checks itself: oracle.Model(param, dst) must give the shipped arrays everywhere but there."""
import os
import shutil
import struct

import numpy as np

from oracle import uvoracle
from oracle.generic_oracle import FP16_FLAG, conv_shapes, parse_param

KINDS = ("tail_bias", "slope")


def model_paths(key):
    base = os.path.join(uvoracle.MODELS_DIR, uvoracle.MODEL_FILES[key])
    return base + ".param", base + ".bin"


def bin_layout(param_path, bin_path):
    """-> [(what, index, byte offset, count)] of the fp32 arrays of the .bin in file order: what = "bias" (index: the
    convolution's) or "slopes" (index: the PReLU's, counted from 0), and the file's length as the walk finds it"""
    layers = parse_param(param_path)
    shapes = {n: (co, ci, k, b) for n, co, ci, k, b in conv_shapes(layers)}
    raw = open(bin_path, "rb").read()
    off, conv, prelu, out = 0, 0, 0, []
    for L in layers:
        if L["type"] == "Convolution":
            co, ci, k, has_bias = shapes[L["name"]]
            n = co * ci * k * k
            flag, = struct.unpack_from("<I", raw, off)
            assert flag in (FP16_FLAG, 0), (L["name"], hex(flag))
            off += 4 + ((2 * n + 3) // 4 * 4 if flag == FP16_FLAG else 4 * n)
            if has_bias:
                out.append(("bias", conv, off, co))
                off += 4 * co
            conv += 1
        elif L["type"] == "PReLU":
            n = int(L["kv"][0])
            out.append(("slopes", prelu, off, n))
            off += 4 * n
            prelu += 1
    assert off == len(raw), ("the walk and the .bin disagree", off, len(raw))
    return out, conv, prelu


def write_mutant_bin(key, dst, kind, amount):
    """shipped .bin of `key` -> dst with one array changed (module docstring); returns (what, index) of that array"""
    assert kind in KINDS, kind
    param, src = model_paths(key)
    layout, n_conv, n_prelu = bin_layout(param, src)
    target = ("bias", n_conv - 1) if kind == "tail_bias" else ("slopes", n_prelu // 2)
    (off, n), = [(o, c) for what, idx, o, c in layout if (what, idx) == target]
    shutil.copyfile(src, dst)
    with open(dst, "r+b") as f:
        f.seek(off)
        a = np.frombuffer(f.read(4 * n), "<f4")
        b = (a + np.float32(amount / 255.0) if kind == "tail_bias" else a * np.float32(1.0 + amount)).astype("<f4")
        assert not np.array_equal(a, b), (key, kind, amount, "changes nothing")
        f.seek(off)
        f.write(b.tobytes())
    # the self-check: through the oracle's own loader, every array is the shipped one except the target
    shipped, mutant = uvoracle.Model(param, src), uvoracle.Model(param, dst)
    assert mutant.bin_consumed == mutant.bin_size == shipped.bin_size
    for i in range(n_conv):
        (w0, b0, t0), (w1, b1, t1) = shipped.conv(i), mutant.conv(i)
        assert t0 == t1 and np.array_equal(w0, w1), (key, kind, "weights of convolution", i)
        if target == ("bias", i):
            assert np.array_equal(b1, b), (key, kind, "the bias was not rewritten")
        else:
            assert np.array_equal(b0, b1), (key, kind, "bias of convolution", i)
    for i in range(n_prelu):
        s0, s1 = shipped.prelu(i), mutant.prelu(i)
        if target == ("slopes", i):
            assert np.array_equal(s1, b), (key, kind, "the slopes were not rewritten")
        else:
            assert np.array_equal(s0, s1), (key, kind, "slopes of PReLU", i)
    return target


def distance_u8(a, b):
    """-> (max |diff| LSB, PSNR dB, share of samples that differ), as check_u8 scores"""
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    mse = float((d.astype(np.float64) ** 2).mean())
    return int(d.max()), (99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))), float((d > 0).mean())
