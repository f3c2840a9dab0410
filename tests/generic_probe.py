"""Probe graphs for tests/test_generic_probes.py: small generic graphs whose arithmetic is EXACT, so that the generic executor's
kernels (csrc/uva_rdb.hip.h, uva_sww.hip.h, uva_generic.hip.h) can be held to a float64 reference bit for bit.

Inputs, weights, biases, slopes and coefficients are small dyadic numbers: every stored activation is then a value fp16 holds
exactly, and every fp32 accumulation adds multiples of one power of two g whose absolute sum stays below 2^24 g -- exact in ANY
order.  A correct kernel of any flavour (direct, k-split, partial sums handed from wave to wave, Winograd F(2,3) with its fp16
transforms) must then return the reference's bits; the audit below proves the premise per probe, weight set and shape.

    Graph            a graph written layer by layer (the Split layers ncnn wants are added when the text is made); the
                     dense-block probes restate the layer pattern of models/4x_Valar_v1.param:4-21
    weights()        sparse dyadic weights, the position of every non-zero by construction: the non-zeros of a convolution walk
                     its k-steps (tap x 32-channel input chunk) in turn, so none is empty and every output channel has 2-3 (the
                     wide convolutions enough to read every input channel)
    Ref              float64 forward of a .param / .bin (parsed by oracle/generic_oracle.py) with the executor's rounding points
                     (the ones of generic_oracle.Model.forward(f16_storage=True)), an Audit, and MUTANTS: one plausible kernel
                     slip each, restated in numpy, for the proofs that the probes can see them
"""
import os
import struct

import numpy as np

from oracle import generic_oracle as go

SLOPE = 0.5
WSETS = (0, 1, 2)


# ---------------------------------------------------------------------------------------------------------- graph writers
class Graph:
    def __init__(self, name):
        self.name = name
        self.ops = []                     # dict(type, name, ins, out, kv, ...) in program order
        self.ch = {"input": 3}
        self.scale = {"input": 1}
        self.ops.append(dict(type="Input", name="input", ins=[], out="input", kv=""))

    def _add(self, typ, name, ins, out, kv, ch, scale, **extra):
        assert out not in self.ch, out
        self.ops.append(dict(type=typ, name=name, ins=list(ins), out=out, kv=kv, **extra))
        self.ch[out], self.scale[out] = ch, scale
        return out

    def conv(self, name, src, cout, k=3, bias=True, act=False, weights="sparse", out=None):
        cin = self.ch[src]
        kv = "0=%d 1=%d" % (cout, k) + (" 4=1" if k == 3 else "") + (" 5=1" if bias else "") + " 6=%d" % (cout * cin * k * k)
        if act:
            kv += " 9=2 -23310=1,%e" % SLOPE
        return self._add("Convolution", name, [src], out or name + "_o", kv, cout, self.scale[src],
                         conv=dict(cout=cout, cin=cin, k=k, bias=bias, act=act, weights=weights))

    def concat(self, name, srcs):
        return self._add("Concat", name, srcs, name + "_o", "", sum(self.ch[s] for s in srcs), self.scale[srcs[0]])

    def add(self, name, a, b):
        return self._add("BinaryOp", name, [a, b], name + "_o", "", self.ch[a], self.scale[a])

    def eltwise(self, name, a, b, ca, cb, out=None):
        return self._add("Eltwise", name, [a, b], out or name + "_o", "0=1 -23301=2,%e,%e" % (ca, cb), self.ch[a], self.scale[a])

    def interp(self, name, src, f=2):
        return self._add("Interp", name, [src], name + "_o", "0=1 1=%e 2=%e" % (f, f), self.ch[src], self.scale[src] * f)

    def prelu(self, name, src):
        return self._add("PReLU", name, [src], name + "_o", "0=%d" % self.ch[src], self.ch[src], self.scale[src], prelu=self.ch[src])

    def pixelshuffle(self, name, src, f, out=None):
        return self._add("PixelShuffle", name, [src], out or name + "_o", "0=%d" % f, self.ch[src] // (f * f), self.scale[src] * f)

    def param_text(self):
        """the .param text: a blob with several readers goes through a Split, every reader taking an alias of its own"""
        readers = {}
        for op in self.ops:
            for b in op["ins"]:
                readers[b] = readers.get(b, 0) + 1
        taken, lines, nblobs = {}, [], 0
        for op in self.ops:
            ins = []
            for b in op["ins"]:
                if readers[b] > 1:
                    taken[b] = taken.get(b, 0) + 1
                    ins.append("%s_s%d" % (b, readers[b] - taken[b]))
                else:
                    ins.append(b)
            lines.append("%-16s %-16s %d 1 %s %s" % (op["type"], op["name"], len(ins), " ".join(ins + [op["out"]]), op["kv"]))
            nblobs += 1
            n = readers.get(op["out"], 0)
            if n > 1:
                lines.append("%-16s %-16s 1 %d %s %s" % ("Split", "split_" + op["out"], n, op["out"],
                                                        " ".join("%s_s%d" % (op["out"], k) for k in range(n))))
                nblobs += n
        assert "output" in self.ch and self.ch["output"] == 3
        return "7767517\n%d %d\n" % (len(lines), nblobs) + "\n".join(ln.rstrip() for ln in lines) + "\n"


def dense_block(g, x, tag):
    """models/4x_Valar_v1.param:6-21 -- x1 = lrelu(conv3(x)), x2 = lrelu(conv3(x, x1)) + conv1(x), x3 = lrelu(conv3(x, x1, x2)),
    x4 = lrelu(conv3(x .. x3)) + x2, result = 0.5 * conv3(x .. x4) + x (there: 0.2)"""
    x1 = g.conv(tag + "c1", x, 32, act=True)
    t2 = g.conv(tag + "c2", g.concat(tag + "cat1", [x, x1]), 32, act=True)
    s2 = g.conv(tag + "c2s", x, 32, k=1, bias=False)
    x2 = g.add(tag + "add2", t2, s2)
    x3 = g.conv(tag + "c3", g.concat(tag + "cat2", [x, x1, x2]), 32, act=True)
    t4 = g.conv(tag + "c4", g.concat(tag + "cat3", [x, x1, x2, x3]), 32, act=True)
    x4 = g.add(tag + "add4", t4, x2)
    y = g.conv(tag + "c5", g.concat(tag + "cat4", [x, x1, x2, x3, x4]), 64)
    return g.eltwise(tag + "sum", y, x, 0.5, 1.0)


def select_tail(g, src, f=4):
    """every probe's way out: a 1x1 convolution that picks 3 f^2 channels (one +-1 each: no bit is added) and a PixelShuffle
    that lays them out as the 3-channel result at f times the size -- 48 of the probed layer's channels reach the comparison
    (another 48 with every weight set), where a 3x3 tail of the probes' sparseness would show six"""
    t = g.conv("tail", src, 3 * f * f, k=1, bias=False, weights="select", out=None if f > 1 else "output")
    return g.pixelshuffle("shuffle", t, f, out="output") if f > 1 else t


def u8_tail(g, src):
    """the u8 route's way out: the graph's last convolution must be a 3x3 one with 3 outputs for the executor to write the frame's
    bytes from its epilogue (GConvArgs::u8dst); weights +-2^-k around a bias near 0.5 keep most samples inside [0, 1]"""
    return g.conv("tail", src, 3, weights="u8tail", out="output")


def g_dense(blocks=1, double_sum=False, u8=False):
    g = Graph("dense%d%s%s" % (blocks, "_sum2" if double_sum else "", "_u8" if u8 else ""))
    head = g.conv("head", "input", 64)
    x = head
    for k in range(blocks):
        x = dense_block(g, x, "b%d" % k)
    if double_sum:                        # models/4x_Valar_v1.param:55-56: a second sum behind the block's, the head's result again
        x = g.eltwise("sum2", x, head, 1.0, 0.5)
    u8_tail(g, x) if u8 else select_tail(g, x)
    return g


def g_scale2_u8():
    """Interp 2x, 64 -> 64 with activation, 64 -> 3: the folded Interp and the u8 epilogue at twice the size"""
    g = Graph("scale2_u8")
    u8_tail(g, g.conv("mid", g.interp("up", g.conv("head", "input", 64)), 64, act=True))
    return g


def g_conv(cin, cout, k=3, act=False, sum_order=None, tail_f=4):
    """one convolution cin -> cout between a 3 -> cin head and the selecting tail; sum_order "ab": Eltwise(conv, head) with
    coefficients 0.5 / 2.0, "ba": Eltwise(head, conv) with the same -- the convolution's result meets another coefficient"""
    g = Graph("conv%d_%dto%d%s%s" % (k, cin, cout, "_act" if act else "", "_sum" + sum_order if sum_order else ""))
    head = g.conv("head", "input", cin)
    y = g.conv("mid", head, cout, k=k, act=act)
    if sum_order:
        assert cin == cout
        y = g.eltwise("sum", y, head, 0.5, 2.0) if sum_order == "ab" else g.eltwise("sum", head, y, 0.5, 2.0)
    select_tail(g, y, tail_f)
    return g


def g_interp():
    """head, nearest 2x Interp, 64 -> 64 with activation (g_conv3_sw's UP form folds the Interp into its row DMA), tail at 2x"""
    g = Graph("interp")
    select_tail(g, g.conv("mid", g.interp("up", g.conv("head", "input", 64)), 64, act=True), f=2)
    return g


def g_prelu_axpby():
    """PReLU with per-channel dyadic slopes (one above 1, one negative, a zero) and a sum no convolution can take into its
    epilogue (the head has two readers, the PReLU is no convolution): g_prelu, g_axpby"""
    g = Graph("prelu_axpby")
    head = g.conv("head", "input", 48)
    select_tail(g, g.eltwise("sum", g.prelu("prelu", head), head, 0.5, 0.25))
    return g


def g_concat():
    """a three-input Concat (dense chains start with two: this one copies, g_concat_part) feeding 96 -> 48 (cin_pad 96, MBN 3)"""
    g = Graph("concat")
    h = g.conv("head", "input", 32)
    a = g.conv("a", h, 32, act=True)
    b = g.conv("b", h, 32, k=1)
    select_tail(g, g.conv("mid", g.concat("cat", [h, a, b]), 48))
    return g


def g_tall():
    """32 -> 32 and 32 -> 64 for a plane tall enough for g_conv3_lds's 16-row, 8-wave forms (MBN 2 and 4); a plain 3-channel way
    out"""
    g = Graph("tall")
    select_tail(g, g.conv("wide", g.conv("mid", g.conv("head", "input", 32), 32, act=True), 64), f=1)
    return g


# ---------------------------------------------------------------------------------------------------------- weight writer
PRELU_SLOPES = (0.5, 1.5, -0.5, 0.25, 0.0, 1.0, 2.0, 0.125)


def _sparse(rng, cout, cin, k, wset, amp=1.0, per_out=None):
    """+-amp non-zeros walking the convolution's k-steps (tap x 32-channel chunk) in turn: output channel o gets 2 or 3 (more
    where cout is too small to reach every k-step otherwise), each at the NEXT k-step, the channel inside the chunk by `rng`"""
    taps, nchunk = k * k, -(-cin // 32)
    nsteps = taps * nchunk
    w = np.zeros((cout, cin, taps))
    t = 5 * wset + 1
    seen, reads = [0] * nchunk, [0] * cin
    for o in range(cout):
        n = per_out or max(2 + (o + wset) % 2, -(-nsteps // cout), -(-32 * nchunk // cout) if cin > 96 else 0)
        for _ in range(n):
            step = t % nsteps
            t += 1
            tap, chunk = step % taps, step // taps
            lo, hi = 32 * chunk, min(cin, 32 * chunk + 32)
            # the channel inside the chunk: the one read least so far (ties: walking on from a start that moves with the weight
            # set), so that a chunk with 32 or more non-zeros has every input channel read -- what a dense block computes for
            # x1 .. x4 reaches the result through the 192 -> 64 convolution's three non-zeros per output
            width = hi - lo
            order = [(reads[lo + (j + seen[chunk] * 7 + 3 * wset) % width], j) for j in range(width)
                     if w[o, lo + (j + seen[chunk] * 7 + 3 * wset) % width, tap] == 0]
            ci = lo + (min(order)[1] + seen[chunk] * 7 + 3 * wset) % width
            seen[chunk] += 1
            reads[ci] += 1
            w[o, ci, tap] = amp * (1 if rng.integers(2) else -1)
    steps_hit = {(tap, c // 32) for _, c, tap in np.argwhere(w != 0)}
    assert len(steps_hit) == nsteps and (np.abs(w).sum(axis=(1, 2)) > 0).all(), "a k-step or an output channel without a weight"
    return w.reshape(cout, cin, k, k)


def weights(g, wset, u8_amp=2.0 ** -6):
    """-> {conv name: (w [cout][cin][k][k], bias [cout])}, {prelu name: slopes}; float64, every value exact in fp16"""
    rng = np.random.default_rng(1000 * wset + sum(map(ord, g.name)))
    W, S = {}, {}
    for op in g.ops:
        if op["type"] == "Convolution":
            c = op["conv"]
            cout, cin, k = c["cout"], c["cin"], c["k"]
            if c["weights"] == "select":
                w = np.zeros((cout, cin, 1, 1))
                for o in range(cout):
                    w[o, (o + 16 * wset + 5) % cin, 0, 0] = 1 if (o + wset) % 3 else -1
                b = np.zeros(cout)
            elif c["weights"] == "u8tail":
                w = _sparse(rng, cout, cin, k, wset, amp=u8_amp)
                # (not 0.5 itself: 255 y ends in .5 only at y = 0.5, which a sum of exactly zero -- common with weights this
                # sparse -- would then hit every time; off 0.5 a tie needs one particular non-zero sum)
                b = 0.5 + np.array([1, -1, 2])[:cout] * (2.0 ** -4 + 2.0 ** -9)
            else:
                w = _sparse(rng, cout, cin, k, wset)
                b = rng.integers(-2, 3, cout).astype(np.float64) if c["bias"] else np.zeros(cout)
            W[op["name"]] = (w, b)
        elif op["type"] == "PReLU":
            S[op["name"]] = np.array([PRELU_SLOPES[(c + wset) % len(PRELU_SLOPES)] for c in range(op["prelu"])])
    return W, S


def write_probe(g, wset, directory, **kw):
    """<directory>/<name>_w<wset>.param / .bin (fp16 payload, fp32 biases and slopes, ncnn modelbin.cpp) -> the two paths"""
    W, S = weights(g, wset, **kw)
    base = os.path.join(str(directory), "%s_w%d" % (g.name, wset))
    with open(base + ".param", "w") as f:
        f.write(g.param_text())
    with open(base + ".bin", "wb") as f:
        for op in g.ops:
            if op["type"] == "Convolution":
                w, b = W[op["name"]]
                w16 = w.astype(np.float16)
                assert np.array_equal(w16.astype(np.float64), w)
                raw = w16.tobytes()
                f.write(struct.pack("<I", go.FP16_FLAG) + raw + b"\0" * (-len(raw) % 4))
                if op["conv"]["bias"]:
                    f.write(b.astype(np.float32).tobytes())
            elif op["type"] == "PReLU":
                f.write(S[op["name"]].astype(np.float32).tobytes())
    return base + ".param", base + ".bin"


def probe_input(h, w, seed, u8=False):
    """float route: f32 [3][h][w] of -1 / 0 / 1 (g_input_f32 only converts); u8 route: a frame of bytes 0 / 255 (exactly 0.0 / 1.0)"""
    rng = np.random.default_rng(seed)
    if u8:
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(-1, 2, (3, h, w)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- the audit
def _low_bit(a):
    """exponent of the lowest set bit over all non-zero values of a (the largest power of two every value is a multiple of)"""
    a = np.abs(np.asarray(a, np.float64).ravel())
    v = a * 2.0 ** 40
    if v.size and float(v.max()) < 2.0 ** 62 and bool((v == np.floor(v)).all()):      # the probes' values: one pass, the OR of all of them
        bits = int(np.bitwise_or.reduce(v.astype(np.int64)))
        return None if bits == 0 else (bits & -bits).bit_length() - 1 - 40
    a = a[a != 0]
    if a.size == 0:
        return None
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
    return int((e - 53 + tz).min())


def _f16_exact(a):
    with np.errstate(over="ignore"):
        return bool(np.array_equal(np.asarray(a, np.float64).astype(np.float16).astype(np.float64), a))


class Audit:
    """what licenses array_equal: `blobs` {name: (every value survives fp16, significant bits = log2(max|v| / granularity))},
    `sums` {layer: order-independent in fp32 (terms multiples of 2^g, sum of |terms| < 2^24 * 2^g)}, `wino` {conv: the F(2,3)
    transforms exact too}"""

    def __init__(self):
        self.blobs, self.sums, self.wino = {}, {}, {}

    def blob(self, name, v):
        g = _low_bit(v)
        bits = 0.0 if g is None else float(np.log2(np.abs(v).max() / 2.0 ** g)) + 1
        ok, b0 = self.blobs.get(name, (True, 0.0))       # (one Audit may see several planes: a verdict holds for all of them)
        self.blobs[name] = (ok and _f16_exact(v), max(bits, b0))

    def terms(self, name, gexp, abs_sum_max):
        self.sums[name] = self.sums.get(name, True) and (gexp is None or abs_sum_max < 2.0 ** (24 + gexp))

    def winograd(self, name, ok):
        self.wino[name] = self.wino.get(name, True) and ok

    def bad(self, skip_blobs=()):
        return ([("blob", k) for k, (ok, _) in self.blobs.items() if not ok and k not in skip_blobs] +
                [("sum", k) for k, ok in self.sums.items() if not ok] + [("wino", k) for k, ok in self.wino.items() if not ok])


def wino_audit(x, w, b):
    """g_conv3_sww's arithmetic (csrc/uva_sww.hip.h:8-12, pack_generic_wino in csrc/uva_generic.cpp): per filter row the taps
    become U = g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2 in fp16; the input columns d0..d3 = 2p - 1 .. 2p + 2 become
    V = d0 - d2, d1 + d2, d2 - d1, d1 - d3 in fp16; M_j = sum U_j V_j in fp32; out = (M0 + M1) + M2, (M1 - M2) - M3 in fp32.
    Exact if every U and V survives fp16 and the M sums and their combinations are order-independent.  V is taken at EVERY column
    offset (a superset of the pairs the kernel forms: no assumption about where a strip starts)."""
    c, h, wd = x.shape
    xp = np.zeros((c, h, wd + 4))
    xp[:, :, 2:-2] = x
    V = [xp[:, :, :-2] - xp[:, :, 2:], xp[:, :, :-1] + xp[:, :, 1:], xp[:, :, 1:] - xp[:, :, :-1]]
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]
    U = [g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2]
    if not all(_f16_exact(v) for v in V) or not all(_f16_exact(u) for u in U):
        return False
    gv, gu = min(_low_bit(v) or 0 for v in V), min(x for x in (_low_bit(u) for u in U) if x is not None)
    gb = _low_bit(b)
    gexp = min(gv + gu, gb if gb is not None else 99)
    vmax = max(float(np.abs(v).max()) for v in V)
    usum = max(float(np.abs(u).sum(axis=(1, 2)).max()) for u in U)         # per output channel: over input channels and filter rows
    return 4 * vmax * usum + float(np.abs(b).max()) < 2.0 ** (24 + gexp)


# ---------------------------------------------------------------------------------------------------------- float64 reference
def _conv64(x, w, b, k):
    """stride-1 'same' convolution in float64: a loop over the non-zero weights where they are few (the probes), one matrix
    product per tap otherwise -- neither is generic_oracle's im2col + tensordot in float32"""
    c, h, wd = x.shape
    cout = w.shape[0]
    p = k // 2
    xp = np.zeros((c, h + 2 * p, wd + 2 * p))
    xp[:, p:p + h, p:p + wd] = x
    out = np.zeros((cout, h, wd))
    nz = np.argwhere(w != 0)
    if len(nz) <= 2048 and len(nz) * 4 < w.size:
        for o, ci, dy, dx in nz:
            out[o] += w[o, ci, dy, dx] * xp[ci, dy:dy + h, dx:dx + wd]
    else:
        for dy in range(k):
            for dx in range(k):
                out += np.tensordot(w[:, :, dy, dx], xp[:, dy:dy + h, dx:dx + wd], axes=1)
    return out + b[:, None, None]


MUTANTS = ("kstep", "halo_col", "seg_row", "last_row", "preact", "swap_sum")


class Ref:
    """float64 forward of a .param / .bin.  mutant: dict(kind=one of MUTANTS, layer=name, ...):
        kstep     convolution `layer` skips k-step (tap, chunk): one tap of one 32-channel input chunk, all outputs
        halo_col  ... reads input column `col` as zero where it is the LEFT neighbour of output column col + 1 (the halo column
                  just outside a strip that starts at col + 1)
        seg_row   ... reads input row `row` as zero for output row row + 1 (the row above a segment's first output row)
        last_row  the result of `layer` has its last row taken from the row above
        preact    the sum `layer` (x4 = lrelu(conv) + x2) is applied before the activation of the convolution in front of it
        swap_sum  the Eltwise `layer` multiplies its operands with each other's coefficient"""

    def __init__(self, param_path, bin_path):
        m = go.Model(param_path, bin_path)
        self.layers = m.layers
        self.w = {k: v.astype(np.float64) for k, v in m.w.items()}
        self.b = {k: v.astype(np.float64) for k, v in m.b.items()}
        self.slopes = {k: v.astype(np.float64) for k, v in m.slopes.items()}

    def forward(self, x, f16_storage=True, audit=None, mutant=None, wino=()):
        """x: [3][h][w] -> float64 [3][h*s][w*s]; wino: names of the convolutions g_conv3_sww takes (audited as such)"""
        def q(a):
            return a.astype(np.float16).astype(np.float64) if f16_storage else a
        mu = mutant or {}
        at = lambda L: mu.get("layer") == L["name"]            # noqa: E731
        blobs, pre = {}, {}
        for L in self.layers:
            raw = None                    # the layer's result before its fp16 rounding, where it has one
            t, kv, ins, outs = L["type"], L["kv"], L["ins"], L["outs"]
            if t == "Input":
                raw = np.asarray(x, np.float64)
                y = q(raw)
            elif t == "Split":
                for o in outs:
                    blobs[o] = blobs[ins[0]]
                continue
            elif t == "Convolution":
                a, w, b, k = blobs[ins[0]], self.w[L["name"]], self.b[L["name"]], int(kv[1])
                if f16_storage:
                    w = q(w)
                if at(L) and mu["kind"] == "kstep":
                    w = w.copy()
                    w[:, 32 * mu["chunk"]:32 * mu["chunk"] + 32, mu["tap"] // k, mu["tap"] % k] = 0
                y = _conv64(a, w, b, k)
                if at(L) and mu["kind"] == "halo_col" and mu["col"] + 1 < a.shape[2]:
                    a2 = a.copy()
                    a2[:, :, mu["col"]] = 0
                    y[:, :, mu["col"] + 1] = _conv64(a2, w, b, k)[:, :, mu["col"] + 1]
                if at(L) and mu["kind"] == "seg_row" and mu["row"] + 1 < a.shape[1]:
                    a2 = a.copy()
                    a2[:, mu["row"]] = 0
                    y[:, mu["row"] + 1] = _conv64(a2, w, b, k)[:, mu["row"] + 1]
                if audit is not None:
                    gw, ga, gb = _low_bit(w), _low_bit(a), _low_bit(b)
                    gexp = None if gw is None or ga is None else gw + ga
                    if gb is not None:
                        gexp = gb if gexp is None else min(gexp, gb)
                    audit.terms(L["name"], gexp, float(_conv64(np.abs(a), np.abs(w), np.abs(b), k).max()))
                    if L["name"] in wino:
                        audit.winograd(L["name"], wino_audit(a, w, b))
                pre[outs[0]] = y
                if int(kv.get(9, 0)) == 2:
                    y = np.where(y > 0, y, y * go._arr(kv, -23310)[0])
                raw = y
                y = q(y)
            elif t == "Concat":
                y = np.concatenate([blobs[i] for i in ins], axis=0)
            elif t in ("BinaryOp", "Eltwise"):
                c = [1.0, 1.0] if t == "BinaryOp" else (go._arr(kv, -23301) or [1.0, 1.0])
                c = [float(np.float32(v)) for v in c]
                if at(L) and mu["kind"] == "swap_sum":
                    c = c[::-1]
                a, b = blobs[ins[0]], blobs[ins[1]]
                y = a * c[0] + b * c[1]
                if at(L) and mu["kind"] == "preact":
                    v = pre[ins[0]] + b
                    y = np.where(v > 0, v, v * SLOPE)
                if audit is not None:
                    ga, gb = _low_bit(a * c[0]), _low_bit(b * c[1])
                    gs = [v for v in (ga, gb) if v is not None]
                    audit.terms(L["name"], min(gs) if gs else None, float((np.abs(a * c[0]) + np.abs(b * c[1])).max()))
                raw = y
                y = q(y)
            elif t == "Interp":
                s = int(float(kv.get(1, 1.0)))
                y = np.repeat(np.repeat(blobs[ins[0]], s, axis=1), s, axis=2)
            elif t == "PReLU":
                a = blobs[ins[0]]
                raw = np.where(a < 0, a * self.slopes[L["name"]][:, None, None], a)
                y = q(raw)
            elif t == "PixelShuffle":
                f = int(kv.get(0, 1))
                a = blobs[ins[0]]
                c, h, w = a.shape
                y = np.zeros((c // (f * f), h * f, w * f))
                for ch in range(c):                       # PyTorch order: input channel (o f + i) f + j -> output o at (y f + i, x f + j)
                    y[ch // (f * f), (ch // f) % f::f, ch % f::f] = a[ch]
            else:
                raise ValueError("layer type " + t)
            if at(L) and mu["kind"] == "last_row" and y.shape[1] >= 2:
                y = y.copy()
                y[:, -1] = y[:, -2]
            if audit is not None and raw is not None:
                audit.blob(outs[0], raw)
            blobs[outs[0]] = y
        return blobs["output"]

    def u8_values(self, img, **kw):
        """u8 HWC frame -> float64 HWC 255 * result (before rounding): apply_model's arithmetic on one plane"""
        x = q16(img.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))
        return self.forward(x, **kw).transpose(1, 2, 0) * 255.0


def q16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def to_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def tiled_u8(ref, img, ts, border=10, swap_border_of=None, **kw):
    """the reference's tile loop (upscale_processing.tile_window) over Ref: -> 255 * result as float64 HWC, pasted cores.
    swap_border_of = k: MUTANT -- plane k's left border columns are the ones of the plane to its right (a batch that hands a
    plane its neighbour's rows)"""
    from upscale_video_amd import upscale_processing as up
    h, w, _ = img.shape
    s = None
    out = None
    k = 0
    for ty in range(-(-h // ts)):
        for tx in range(-(-w // ts)):
            (y0, y1, x0, x1), (top, bottom, left, right) = up.tile_window(ts, ty, tx, h, w, border)
            tile = np.ascontiguousarray(img[y0 - top:y1 + bottom, x0 - left:x1 + right])
            if swap_border_of == k and left and x1 + left <= w:
                tile = tile.copy()
                tile[:, :left] = img[y0 - top:y1 + bottom, x1:x1 + left]
            v = ref.u8_values(tile, **kw)
            if out is None:
                s = v.shape[0] // tile.shape[0]
                out = np.zeros((s * h, s * w, 3))
            out[s * y0:s * y1, s * x0:s * x1] = v[s * top:s * (top + y1 - y0), s * left:s * (left + x1 - x0)]
            k += 1
    return out
