"""Every oracle comparison of the -m gpu tests leaves its MEASURED distance here, next to the bar it was held to
("state the parity slack as measured + margin, and show it").

    from parity_report import check_u8, check_f32

    check_u8("tiled 2x 70x75 t32", got, want, vs="fp32 oracle", max_lsb=2, min_psnr=50)

records max |diff| (LSB), PSNR (dB) and the share of differing samples, THEN asserts the bars (check_u16: u16 frames, scored
in codes; check_f32: float blobs).  conftest.py writes the
records to gpurun_out/parity_report.json at the end of the session and prints one line per record in pytest's terminal
summary (so that the driver's `-q` log shows them); tools/parity_slack.py turns a report into tests/golden/parity_slack.json,
the committed measurements the product-mode bars are derived from (bar = measured maximum + margin, per model and route).
"""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = []
_SLACK = None


def psnr_u8(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean()) if d.size else 0.0
    return 99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def slack(model, route, what, fallback):
    """Bar for `what` ("u8_differ_share", "layer_rel", "f32_abs") of `model` on `route` from the committed sweep:
    measured maximum + margin (tests/golden/parity_slack.json, written by tools/parity_slack.py from a GPU run's report);
    `fallback` where the file has no entry (a new model / route: the round number it replaces)."""
    global _SLACK
    if _SLACK is None:
        try:
            _SLACK = json.load(open(os.path.join(ROOT, "tests", "golden", "parity_slack.json")))
        except (OSError, ValueError):
            _SLACK = {}
    e = _SLACK.get("bars", {}).get(f"{model}/{route}/{what}")
    return float(e["bar"]) if e else fallback


LARGE_SAMPLES = 10 ** 6     # a comparison of at least this many samples is "large": counting noise no longer sets its distance


def size_class(samples):
    return "large" if samples is not None and samples >= LARGE_SAMPLES else "small"


def fp32_bar(model, route, input_class=None, samples=None):
    """Bars of a comparison with the fp32 oracle (kernel-independent) as keyword arguments of check_u8: the measured worst
    case of `model` on `route` -/+ a margin (tests/golden/parity_slack.json "fp32_bars", tools/parity_slack.py), never looser
    than the fixed bars they replace; those fixed bars where nothing has been measured yet.
    With `input_class` (the content of the frame as the CALL SITE knows it: "smooth", "random", ...; never read off a record's
    name) and `samples` (how many are compared: size_class) the entry "{model}/{route}/{input_class}/{size}" applies where there
    is one -- white noise then no longer sets the bar of a smooth 2160p frame -- and the "{model}/{route}" entry where there
    is none.  A class entry only ever tightens: each field is the stricter of the two."""
    slack("", "", "", 0)                                    # loads the file
    bars = _SLACK.get("fp32_bars", {})
    e = bars.get(f"{model}/{route}")
    chain = model == "chain"
    if not e:
        out = {"max_lsb": 3 if chain else 2, "min_psnr": 48.0 if chain else 50.0}
    else:
        out = {"max_lsb": int(e["max_lsb"]), "min_psnr": float(e["min_psnr_db"]), "max_share": float(e["max_differ_share"])}
    c = bars.get(f"{model}/{route}/{input_class}/{size_class(samples)}") if input_class is not None else None
    if c:
        out["max_lsb"] = min(out["max_lsb"], int(c["max_lsb"]))
        out["min_psnr"] = max(out["min_psnr"], float(c["min_psnr_db"]))
        out["max_share"] = min(out.get("max_share", 1.0), float(c["max_differ_share"]))
    return out


def record(name, **fields):
    rec = {"name": name}
    rec.update({k: (round(v, 6) if isinstance(v, float) else v) for k, v in fields.items()})
    RECORDS.append(rec)
    return rec


STRUCTURE_MIN = 48          # lines shorter than this many pixels say nothing about structure
STRUCTURE_Z = 12.0          # bar on the line statistic below (calibration: profiles/r06_structure_calibration.txt)
STRUCTURE_HALF = 12         # the local baseline of a line = median over this many lines either side


def _line_excess(line_mean, n, frame_mean):
    """How far each line's (row's / column's) mean |diff| stands above its neighbourhood, in units of the standard error
    a line of n independent 0/1 samples would have: z = (c_j - median(c_{j-12..j+12})) / sqrt(max(baseline, frame mean, 1/n) / n).
    The running median follows what the picture does to the error rate (it varies smoothly with the content); a schedule
    bug does not: one wrong column or row, a plane edge, every 74th column."""
    k = len(line_mean)
    if k < 2 * STRUCTURE_HALF + 1:
        return np.zeros(k)
    pad = np.pad(line_mean, STRUCTURE_HALF, mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(pad, 2 * STRUCTURE_HALF + 1)
    base = np.median(win, axis=1)
    return (line_mean - base) / np.sqrt(np.maximum(np.maximum(base, frame_mean), 1.0 / n) / n)


def structure_u8(d):
    """|diff| [h][w][c] -> {"col_z", "row_z", "col_at", "row_at", "col_ratio", "row_ratio"} or None for small frames.
    No spatial structure means: no single row or column carries visibly more error than its neighbours."""
    if d.ndim != 3 or d.shape[0] < STRUCTURE_MIN or d.shape[1] < STRUCTURE_MIN:
        return None
    m = float(d.mean())
    col = d.mean(axis=(0, 2), dtype=np.float64)
    row = d.mean(axis=(1, 2), dtype=np.float64)
    zc = _line_excess(col, d.shape[0] * d.shape[2], m)
    zr = _line_excess(row, d.shape[1] * d.shape[2], m)
    floor = max(m, 1e-9)
    return {"col_z": float(zc.max()), "col_at": int(zc.argmax()), "row_z": float(zr.max()), "row_at": int(zr.argmax()),
            "col_ratio": float(col.max() / floor), "row_ratio": float(row.max() / floor)}


def check_u8(name, got, want, vs, max_lsb, min_psnr=None, max_share=None, model=None, route=None, structure=True,
             input_class=None):
    """u8 frames: record, then hold to the bars (max |diff| in LSB, PSNR in dB, share of samples that differ) and -- on
    frames of at least 48 x 48 -- to "the error has no spatial structure" (structure_u8: a row or column whose mean |diff|
    stands STRUCTURE_Z standard errors above its neighbours fails, whatever the LSB and dB bars say: round 5's folded-strip
    bug was one wrong column in 74 inside <= 2 LSB / >= 50 dB).  `input_class` (what the frame holds: "smooth", "random", ...)
    goes into the record: tools/parity_slack.py derives the fp32 bars per class from it (fp32_bar)."""
    assert got.shape == want.shape and got.dtype == np.uint8, (name, got.shape, want.shape, got.dtype)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    worst = int(d.max()) if d.size else 0
    share = float((d > 0).mean()) if d.size else 0.0
    p = psnr_u8(got, want)
    st = structure_u8(d) if structure else None
    record(name, kind="u8", vs=vs, model=model, route=route, input_class=input_class, samples=int(d.size), max_lsb=worst,
           psnr_db=p, differ_share=share, bar_max_lsb=max_lsb, bar_min_psnr_db=min_psnr, bar_max_share=max_share, structure=st,
           bar_structure_z=(STRUCTURE_Z if st else None))
    if st:
        assert st["col_z"] <= STRUCTURE_Z, (name, vs, "structured error: column", st["col_at"], "stands", st["col_z"], "s.e. above its neighbours", st)
        assert st["row_z"] <= STRUCTURE_Z, (name, vs, "structured error: row", st["row_at"], "stands", st["row_z"], "s.e. above its neighbours", st)
    assert worst <= max_lsb, (name, vs, "max |diff|", worst, "bar", max_lsb)
    if min_psnr is not None:
        assert p >= min_psnr, (name, vs, "PSNR", p, "bar", min_psnr)
    if max_share is not None:
        assert share <= max_share, (name, vs, "differing share", share, "bar", max_share)
    return worst, p, share


U16_PRODUCT = "product-mode oracle, u16 codes"    # the vs of the 16-bit route's product-mode records (tools/parity_slack.py)
U16_MAX = 65535


def structure_codes(d):
    """structure_u8 for |diff| in codes (u16 frames): its standard error assumes a sample's variance equals its mean, true of
    u8's 0/1 differences; differences of many codes have a variance of about their mean squared, so |diff| is rescaled by
    mean / variance first (a rescaling the ratios ignore)"""
    if d.ndim != 3 or d.shape[0] < STRUCTURE_MIN or d.shape[1] < STRUCTURE_MIN:
        return None
    v = float(d.var())
    return structure_u8(d * (float(d.mean()) / v) if v > 0 else d)


def score_u16(got, want):
    """u16 frames -> their distance in codes (1 / 65535): max |diff|, RMS, mean signed bias (got - want), share of samples
    that differ, and the share of samples off the clamp ends (0, 65535) that are multiples of 257 -- every one on a route
    that carries 8 bits somewhere (widen(narrow(y)) = 257 rint(y / 257)), about 1 / 257 on a route that keeps 16"""
    d = got.astype(np.int32) - want.astype(np.int32)
    inner = got[(got != 0) & (got != U16_MAX)]
    return {"max_codes": int(np.abs(d).max()) if d.size else 0,
            "rms_codes": float(np.sqrt((d.astype(np.float64) ** 2).mean())) if d.size else 0.0,
            "bias_codes": float(d.mean()) if d.size else 0.0,
            "differ_share": float((d != 0).mean()) if d.size else 0.0,
            "x257_share": float((inner % 257 == 0).mean()) if inner.size else 0.0}


def check_u16(name, got, want, vs, max_codes=None, max_rms=None, max_bias=None, max_x257=None, model=None, route=None,
              structure=True, counterfactual=False):
    """u16 frames, scored in codes (score_u16, and on frames of at least 48 x 48 structure_codes): record, then hold to the
    bars given (max |diff|, RMS and |mean signed bias| in codes, the share of unclamped samples that are multiples of 257).
    counterfactual=True: `got` is what a route that carries 8 bits would give (widen(narrow(y))).  It is recorded with the
    bars, without the structure statistic (quantising smooth content is structured by nature), and must FAIL each depth bar
    given -- RMS and multiples of 257 -- which shows that those bars tell such a route from a 16-bit one."""
    assert got.shape == want.shape and got.dtype == np.uint16 and want.dtype == np.uint16, (name, got.shape, want.shape, got.dtype, want.dtype)
    sc = score_u16(got, want)
    st = structure_codes(np.abs(got.astype(np.int32) - want.astype(np.int32))) if structure and not counterfactual else None
    record(name, kind="u16", vs=vs, model=model, route=route, samples=int(got.size), structure=st,
           bar_max_codes=max_codes, bar_rms_codes=max_rms, bar_bias_codes=max_bias, bar_x257_share=max_x257,
           bar_structure_z=(STRUCTURE_Z if st else None), counterfactual=counterfactual, **sc)
    bars = (("max |diff| codes", "max_codes", max_codes), ("RMS codes", "rms_codes", max_rms), ("|bias| codes", "bias_codes", max_bias),
            ("x257 share", "x257_share", max_x257))
    fails = [(what, sc[key], bar) for what, key, bar in bars if bar is not None and abs(sc[key]) > bar]
    if counterfactual:
        depth = [(what, sc[key], bar) for what, key, bar in bars if key in ("rms_codes", "x257_share") and bar is not None]
        assert depth and all(abs(v) > bar for _, v, bar in depth), (name, vs, "the 8-bit counterfactual passes a depth bar", depth, sc)
        return sc
    if st:
        assert st["col_z"] <= STRUCTURE_Z, (name, vs, "structured error: column", st["col_at"], "stands", st["col_z"], "s.e. above its neighbours", st)
        assert st["row_z"] <= STRUCTURE_Z, (name, vs, "structured error: row", st["row_at"], "stands", st["row_z"], "s.e. above its neighbours", st)
    assert not fails, (name, vs, fails, sc)
    return sc


def check_f32(name, got, want, vs, max_abs, model=None, route=None, what="f32_abs", scale=None):
    """float blobs: record max |diff| (and, with `scale`, relative to the blob's range), then hold to max_abs"""
    err = float(np.abs(got - want).max()) if got.size else 0.0
    record(name, kind="f32", vs=vs, model=model, route=route, what=what, max_abs_err=err,
           rel_to_range=(err / scale if scale else None), bar_max_abs=float(max_abs))
    assert err <= max_abs, (name, vs, "max |err|", err, "bar", max_abs)
    return err


def write(path=None):
    if not RECORDS:
        return None
    out_dir = os.path.join(ROOT, "gpurun_out")
    path = path or os.path.join(out_dir, "parity_report.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump({"records": RECORDS}, f, indent=1)
    except OSError:
        return None
    return path


def summary_lines():
    for r in RECORDS:
        if r.get("kind") == "u8":
            st = r.get("structure")
            yield ("parity %-58s vs %-34s max %d LSB (bar %s)  PSNR %6.2f dB (bar %s)  differ %.3f %% (bar %s)%s" % (
                r["name"][:58], r["vs"][:34], r["max_lsb"], r["bar_max_lsb"], r["psnr_db"], r["bar_min_psnr_db"],
                100 * r["differ_share"], ("%.1f %%" % (100 * r["bar_max_share"])) if r["bar_max_share"] is not None else "-",
                ("  structure z col %.1f row %.1f (bar %.0f)" % (st["col_z"], st["row_z"], r["bar_structure_z"])) if st else "")
                   + (("  [%s/%s]" % (r["input_class"], size_class(r.get("samples")))) if r.get("input_class") else ""))
        elif r.get("kind") == "u16":
            st = r.get("structure")
            bar = lambda k, f, m=1: ("bar " + f % (m * r[k])) if r.get(k) is not None else "bar -"   # noqa: E731
            yield ("parity %-58s vs %-34s max %d codes (%s)  RMS %.2f codes (%s)  bias %+.2f (%s)  differ %.1f %%  "
                   "x257 %.2f %% (%s)%s%s" % (
                       r["name"][:58], r["vs"][:34], r["max_codes"], bar("bar_max_codes", "%.0f"), r["rms_codes"],
                       bar("bar_rms_codes", "%.2f"), r["bias_codes"], bar("bar_bias_codes", "%.2f"), 100 * r["differ_share"],
                       100 * r["x257_share"], bar("bar_x257_share", "%.2f %%", 100),
                       ("  structure z col %.1f row %.1f (bar %.0f)" % (st["col_z"], st["row_z"], r["bar_structure_z"])) if st else "",
                       "  8-bit COUNTERFACTUAL (fails its depth bars)" if r.get("counterfactual") else ""))
        elif r.get("kind") == "pair":           # two distances from one reference side by side, no bar (tests/test_parity_bars.py)
            yield ("parity %-58s vs %-34s GPU max %d LSB, %.2f dB, %.3f %%  |  product-mode oracle max %d LSB, %.2f dB, %.3f %%" % (
                r["name"][:58], r["vs"][:34], r["gpu_max_lsb"], r["gpu_psnr_db"], 100 * r["gpu_differ_share"],
                r["oracle_max_lsb"], r["oracle_psnr_db"], 100 * r["oracle_differ_share"]))
        else:
            yield ("parity %-58s vs %-34s max |err| %.3e (bar %.3e)%s" % (
                r["name"][:58], r["vs"][:34], r["max_abs_err"], r["bar_max_abs"],
                ("  = %.2e of the range" % r["rel_to_range"]) if r.get("rel_to_range") else ""))
