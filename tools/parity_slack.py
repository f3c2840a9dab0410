#!/usr/bin/env python3
"""gpurun_out/parity_report.json (written by `pytest tests -m gpu`, tests/parity_report.py) -> tests/golden/parity_slack.json:
the bars of the PRODUCT-MODE comparisons (GPU against the oracle run with the kernel's own rounding points), per model and
route, as MEASURED MAXIMUM + MARGIN instead of a round number:

    u8_differ_share  share of u8 samples that differ (by one level)          margin: one point (0.01)
    layer_rel        per-layer activations, max |err| / the layer's range    margin: 5e-4
    f32_abs          pre-quantisation f32 output, max |err|                  margin: 5e-4
    u16/rms_codes    the 16-bit route's u16 output, RMS in codes             margin: MARGIN["rms_codes"]
    u16/max_codes    the 16-bit route's u16 output, max |diff| in codes      margin: MARGIN["max_codes"]

The u16 bars come from the records whose vs is U16_VS (tests/parity_report.py U16_PRODUCT; counterfactual records left out),
and are capped: RMS at half an 8-bit hop's, max |diff| at the float route's f32_abs bar of the same model in codes (the bar
the route borrowed before it had its own).

    python tools/parity_slack.py [report.json ...]      several reports (boxes, sweeps): the maximum over all of them
    python tools/parity_slack.py --out PATH [...]       write PATH instead of tests/golden/parity_slack.json

The fp32 bars (GPU against the fp32 oracle, independent of the kernel) are the measured worst case -/+ a margin per model and
route ("fp32_bars"), capped at the round numbers they replace (<= 2 LSB, >= 50 dB), and refined per INPUT CLASS: records
that carry `input_class` (tests/parity_report.py check_u8; the call site says what its frame holds) are grouped by
"{model}/{route}/{input_class}/{size}" as well, size = "large" from LARGE_SAMPLES compared samples on, else "small":

    large   min PSNR - 1.0 dB, max share x 1.25   one build and one seeded frame reproduce their distance bit for bit, so the
                                                  margin covers a legitimate change of summation order (the largest so far,
                                                  direct -> Winograd F(2,3), moved 0.05 dB; the folded-strip bug moved 1.4 dB)
    small   min PSNR - 2.0 dB, max share + 0.015  a 24 x 24 window is 1 728 samples: counting noise dominates

A class entry is never looser than the "{model}/{route}" entry it refines, field by field.  Records without `input_class`
(every report older than the classes) feed the "{model}/{route}" entries only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16_VS = "product-mode oracle, u16 codes"
MARGIN = {"u8_differ_share": 0.01, "layer_rel": 5e-4, "f32_abs": 5e-4, "rms_codes": 1.0, "max_codes": 33.0}
# the round numbers of round 4 the derived bars replaced (tests/test_gpu_parity.py's fallbacks): never exceeded.  u16: half
# the RMS of an 8-bit hop on content spread over the codes (257 / sqrt(12) / 2); max |diff|: the float route's round number
# in codes, unless that model's f32_abs bar is there to cap it
FIXED = {"u8_differ_share": {"1x": 5e-2, "wino": 8e-2}, "layer_rel": {"1x": 2e-3, "wino": 3e-3}, "f32_abs": {"1x": 3e-3, "wino": 4e-3},
         "rms_codes": {"1x": 37.0, "wino": 37.0}, "max_codes": {"1x": 3e-3 * 65535, "wino": 4e-3 * 65535}}
FP32_PSNR_MARGIN, FP32_SHARE_MARGIN = 2.0, 0.015
LARGE_SAMPLES = 10 ** 6
FP32_LARGE_PSNR_MARGIN, FP32_LARGE_SHARE_FACTOR = 1.0, 1.25


def size_class(samples):
    """"large" from LARGE_SAMPLES compared samples on (tests/parity_report.py size_class is this rule: a test holds the two together)"""
    return "large" if samples is not None and samples >= LARGE_SAMPLES else "small"


def _fp32_add(table, key, r):
    e = table.setdefault(key, {"comparisons": 0, "max_lsb": 0, "min_psnr_db": 99.0, "max_differ_share": 0.0})
    e["comparisons"] += 1
    e["max_lsb"] = max(e["max_lsb"], r["max_lsb"])
    e["min_psnr_db"] = round(min(e["min_psnr_db"], r["psnr_db"]), 2)
    e["max_differ_share"] = round(max(e["max_differ_share"], r["differ_share"]), 5)


def main(paths, dst=None):
    paths = paths or [os.path.join(ROOT, "gpurun_out", "parity_report.json")]
    worst, count, fp32, fp32_class = {}, {}, {}, {}
    for p in paths:
        for r in json.load(open(p))["records"]:
            if not r.get("model") or not r.get("route"):
                continue
            if r["kind"] == "u16":
                if r["vs"] == U16_VS and not r.get("counterfactual"):
                    for what in ("rms_codes", "max_codes"):
                        key = f"{r['model']}/{r['route']}/{what}"
                        worst[key] = max(worst.get(key, 0.0), r[what])
                        count[key] = count.get(key, 0) + 1
            elif "product rounding mode" in r["vs"]:
                if r["kind"] == "u8":
                    key, val = f"{r['model']}/{r['route']}/u8_differ_share", r["differ_share"]
                elif r.get("what") == "layer_rel":
                    key, val = f"{r['model']}/{r['route']}/layer_rel", r["rel_to_range"]
                else:
                    key, val = f"{r['model']}/{r['route']}/f32_abs", r["max_abs_err"]
                worst[key] = max(worst.get(key, 0.0), val)
                count[key] = count.get(key, 0) + 1
            elif r["kind"] == "u8" and r["vs"].startswith("fp32 oracle"):
                _fp32_add(fp32, f"{r['model']}/{r['route']}", r)
                if r.get("input_class"):
                    _fp32_add(fp32_class, f"{r['model']}/{r['route']}/{r['input_class']}/{size_class(r.get('samples'))}", r)
    bars = {}
    for key in sorted(worst, key=lambda k: k.endswith("_codes")):             # the u16 caps read the float bars
        what = key.rsplit("/", 1)[1]
        cap = FIXED[what]["1x" if key.startswith("1x/") else "wino"]         # a recalibration can only tighten
        if what == "max_codes" and key.split("/")[0] + "/float/f32_abs" in bars:
            cap = round(65535 * bars[key.split("/")[0] + "/float/f32_abs"]["bar"], 1)
        bars[key] = {"measured_max": round(worst[key], 6), "margin": MARGIN[what], "bar": round(min(worst[key] + MARGIN[what], cap), 6),
                     "cap": cap, "comparisons": count[key]}
    # the kernel-independent bars (GPU against the fp32 oracle), per model and route: measured worst case -/+ a margin, and never
    # looser than the round numbers they replace (<= 2 LSB, >= 50 dB; the chain: <= 3 LSB, >= 48 dB) -- VERDICT r5 item 1c
    fp32_bars = {}
    for k, e in sorted(fp32.items()):
        chain = k.startswith("chain/")
        fp32_bars[k] = {"max_lsb": min(3 if chain else 2, e["max_lsb"] + 1),
                        "min_psnr_db": round(max(48.0 if chain else 50.0, e["min_psnr_db"] - FP32_PSNR_MARGIN), 2),
                        "max_differ_share": round(e["max_differ_share"] + FP32_SHARE_MARGIN, 5)}
    # ... refined per input class; each field the stricter of the class's own figure and the model/route bar above
    for k, e in sorted(fp32_class.items()):
        base = fp32_bars[k.rsplit("/", 2)[0]]
        large = k.endswith("/large")
        psnr = e["min_psnr_db"] - (FP32_LARGE_PSNR_MARGIN if large else FP32_PSNR_MARGIN)
        share = e["max_differ_share"] * FP32_LARGE_SHARE_FACTOR if large else e["max_differ_share"] + FP32_SHARE_MARGIN
        e["margins"] = ({"psnr_db": FP32_LARGE_PSNR_MARGIN, "differ_share_factor": FP32_LARGE_SHARE_FACTOR} if large else
                        {"psnr_db": FP32_PSNR_MARGIN, "differ_share": FP32_SHARE_MARGIN})
        fp32_bars[k] = {"max_lsb": min(base["max_lsb"], e["max_lsb"] + 1),
                        "min_psnr_db": round(max(base["min_psnr_db"], psnr), 2),
                        "max_differ_share": round(min(base["max_differ_share"], share), 5)}
    fp32.update(fp32_class)
    bars = dict(sorted(bars.items()))
    out = {"about": "product-mode parity bars = measured maximum + margin (tools/parity_slack.py); fp32_bars = the kernel-independent "
                    "bars against the fp32 oracle, measured worst case (fp32_measured) -/+ a margin, capped at the round numbers "
                    "they replace (<= 2 LSB, >= 50 dB); fp32 keys of four parts (model/route/input class/size) refine the model/route "
                    "bar for one class of input and are never looser than it (margins: fp32_class_margins and per entry)",
           "sources": [os.path.relpath(os.path.abspath(p), ROOT) for p in paths], "bars": bars, "fp32_measured": fp32,
           "fp32_bars": fp32_bars, "fp32_margins": {"psnr_db": FP32_PSNR_MARGIN, "differ_share": FP32_SHARE_MARGIN},
           "fp32_class_margins": {"large": {"psnr_db": FP32_LARGE_PSNR_MARGIN, "differ_share_factor": FP32_LARGE_SHARE_FACTOR,
                                            "from_samples": LARGE_SAMPLES},
                                  "small": {"psnr_db": FP32_PSNR_MARGIN, "differ_share": FP32_SHARE_MARGIN}}}
    dst = dst or os.path.join(ROOT, "tests", "golden", "parity_slack.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", dst)
    for k, v in fp32_bars.items():
        print("  fp32 %-36s <= %d LSB, >= %.2f dB, differ <= %.3f" % (k, v["max_lsb"], v["min_psnr_db"], v["max_differ_share"]))
    for k, v in bars.items():
        print("  %-34s measured %.5f + %.4f -> bar %.5f (%d comparisons)" % (k, v["measured_max"], v["margin"], v["bar"], v["comparisons"]))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    main(args, out_path)
