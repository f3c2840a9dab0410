"""tests/parity_report.py's u16 scoring (check_u16) and tools/parity_slack.py's u16 bars, on synthetic frames and records
(no GPU).  The records these tests make go to a list of their own: the session's report holds only real comparisons."""
import importlib.util
import json
import os

import numpy as np
import pytest

import parity_report as pr
import pixfmt16_ref as ref
from conftest import ROOT


@pytest.fixture
def records(monkeypatch):
    mine = []
    monkeypatch.setattr(pr, "RECORDS", mine)
    return mine


def _tool():
    spec = importlib.util.spec_from_file_location("parity_slack", os.path.join(ROOT, "tools", "parity_slack.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_score_u16_known_answers():
    want = np.full((4, 5, 3), 1000, np.uint16)
    got = want.copy()
    got[0, 0, 0] = 1010           # +10
    got[1, 2, 1] = 997            # -3
    got[3, 4, 2] = 1001           # +1
    sc = pr.score_u16(got, want)
    assert sc["max_codes"] == 10
    assert sc["rms_codes"] == pytest.approx(np.sqrt((100 + 9 + 1) / 60))
    assert sc["bias_codes"] == pytest.approx(8 / 60)
    assert sc["differ_share"] == pytest.approx(3 / 60)
    # no wrap-around at the ends of the range
    sc = pr.score_u16(np.full((2, 2, 3), 65535, np.uint16), np.zeros((2, 2, 3), np.uint16))
    assert sc["max_codes"] == 65535 and sc["bias_codes"] == 65535 and sc["rms_codes"] == 65535


def test_x257_share_tells_an_8_bit_hop():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 65536, (200, 300, 3), dtype=np.uint16)
    assert abs(pr.score_u16(y, y)["x257_share"] - 1 / 257) < 1e-3
    assert pr.score_u16(ref.widen(ref.narrow(y)), y)["x257_share"] == 1.0
    # the clamp ends (0 and 65535 are multiples of 257 too) do not count
    ends = np.where(rng.random(y.shape) < 0.5, 0, 65535).astype(np.uint16)
    ends[0, 0, 0] = 1
    assert pr.score_u16(ends, ends)["x257_share"] == 0.0


def test_check_u16_records_and_holds_the_bars(records):
    rng = np.random.default_rng(2)
    want = rng.integers(1000, 64000, (20, 30, 3), dtype=np.uint16)
    got = (want.astype(np.int32) + rng.integers(-3, 4, want.shape)).astype(np.uint16)
    sc = pr.check_u16("synthetic", got, want, vs="somewhere", max_codes=3, max_rms=2.5, max_bias=0.5, max_x257=0.02, model="2x",
                      route="u16")
    r = records[-1]
    assert r["kind"] == "u16" and r["vs"] == "somewhere" and r["model"] == "2x" and r["route"] == "u16"
    assert r["max_codes"] == sc["max_codes"] == 3 and r["bar_rms_codes"] == 2.5 and r["counterfactual"] is False
    assert r["structure"] is None                   # 20 x 30: too small for the line statistic
    for bar in ({"max_codes": 2}, {"max_rms": 1.0}, {"max_bias": -1.0}, {"max_x257": 0.0}):
        with pytest.raises(AssertionError):
            pr.check_u16("synthetic", got, want, vs="somewhere", **bar)
    with pytest.raises(AssertionError):             # wrong dtype: a u8 frame is not scored in codes
        pr.check_u16("synthetic", got.astype(np.uint8), want.astype(np.uint8), vs="somewhere")
    lines = list(pr.summary_lines())
    assert len(lines) == len(records) >= 5
    assert "synthetic" in lines[0] and "codes" in lines[0] and "RMS" in lines[0] and "x257" in lines[0]


def test_check_u16_counterfactual_must_fail_its_depth_bars(records):
    rng = np.random.default_rng(3)
    y = rng.integers(0, 65536, (16, 16, 3), dtype=np.uint16)
    q8 = ref.widen(ref.narrow(y))
    rms8 = pr.score_u16(q8, y)["rms_codes"]
    assert 70 < rms8 < 78                           # 257 / sqrt(12) = 74.2
    pr.check_u16("cf", q8, y, vs="v (counterfactual)", max_rms=0.5 * rms8, max_x257=2 / 257, max_codes=1000, counterfactual=True)
    assert records[-1]["counterfactual"] is True and "COUNTERFACTUAL" in list(pr.summary_lines())[-1]
    for loose in ({"max_rms": 100.0, "max_x257": 2 / 257}, {"max_rms": 10.0, "max_x257": 1.0}, {"max_codes": 10}):
        with pytest.raises(AssertionError, match="counterfactual passes"):
            pr.check_u16("cf", q8, y, vs="v (counterfactual)", counterfactual=True, **loose)


def test_structure_in_codes():
    """Noise of many codes has no structure; one column a few codes worse is structure -- whatever the size of the noise"""
    rng = np.random.default_rng(4)
    for sigma in (0.5, 4.0, 40.0):
        d = np.abs(np.rint(rng.normal(0, sigma, (240, 320, 3)))).astype(np.int32)
        st = pr.structure_codes(d)
        assert st["col_z"] <= pr.STRUCTURE_Z and st["row_z"] <= pr.STRUCTURE_Z, (sigma, st)
        bad = d.copy()
        bad[:, 150] += max(1, int(sigma))           # one column off by about a standard deviation
        st = pr.structure_codes(bad)
        assert st["col_z"] > 2 * pr.STRUCTURE_Z and st["col_at"] == 150, (sigma, st)
        assert st["row_z"] <= pr.STRUCTURE_Z, (sigma, st)
    assert pr.structure_codes(np.zeros((47, 100, 3), np.int32)) is None
    assert pr.structure_codes(np.zeros((60, 100, 3), np.int32))["col_z"] == 0


def test_check_u16_fails_a_structured_error(records):
    rng = np.random.default_rng(5)
    want = rng.integers(2000, 60000, (64, 96, 3), dtype=np.uint16)
    got = (want.astype(np.int32) + np.rint(rng.normal(0, 6, want.shape)).astype(np.int32)).astype(np.uint16)
    pr.check_u16("smooth error", got, want, vs="v", max_codes=100)
    got[17] += 8                                    # one row
    with pytest.raises(AssertionError, match="structured error: row"):
        pr.check_u16("one bad row", got, want, vs="v", max_codes=100)


def _u16(model, rms, mx, vs=pr.U16_PRODUCT, counterfactual=False):
    return {"name": "r", "kind": "u16", "vs": vs, "model": model, "route": "u16", "rms_codes": rms, "max_codes": mx,
            "counterfactual": counterfactual}


def test_parity_slack_derives_the_u16_bars(tmp_path):
    tool = _tool()
    assert tool.U16_VS == pr.U16_PRODUCT            # one vs string for the records the tool reads
    recs = [_u16("2x", 3.0, 50), _u16("2x", 5.5, 40), _u16("2x", 74.0, 128, counterfactual=True),
            _u16("2x", 90.0, 900, vs="fp32 oracle"), _u16("4x", 2.0, 250), _u16("4x", 4.0, 20),
            {"name": "f", "kind": "f32", "vs": "oracle, product rounding mode", "model": "2x", "route": "float",
             "what": "f32_abs", "max_abs_err": 0.001}]
    src = tmp_path / "report.json"
    src.write_text(json.dumps({"records": recs}))
    dst = tmp_path / "slack.json"
    out = tool.main([str(src)], str(dst))
    assert json.loads(dst.read_text()) == json.loads(json.dumps(out))
    bars = out["bars"]
    assert set(bars) == {"2x/float/f32_abs", "2x/u16/rms_codes", "2x/u16/max_codes", "4x/u16/rms_codes", "4x/u16/max_codes"}
    m_rms, m_max = tool.MARGIN["rms_codes"], tool.MARGIN["max_codes"]
    e = bars["2x/u16/rms_codes"]        # the counterfactual and the fp32 comparison are not measurements of the route
    assert e["measured_max"] == 5.5 and e["bar"] == pytest.approx(5.5 + m_rms) and e["comparisons"] == 2
    e = bars["2x/u16/max_codes"]        # capped at the float route's bar of the model, in codes
    assert e["measured_max"] == 50 and e["cap"] == pytest.approx(65535 * 0.0015, abs=0.1)
    assert e["bar"] == pytest.approx(min(50 + m_max, e["cap"]))
    e = bars["4x/u16/max_codes"]        # no float bar for 4x here: the round number
    assert e["cap"] == pytest.approx(4e-3 * 65535) and e["bar"] == pytest.approx(e["cap"])
    assert bars["4x/u16/rms_codes"]["bar"] == pytest.approx(4.0 + m_rms)
    assert all(b["bar"] <= tool.FIXED["rms_codes"]["wino"] for k, b in bars.items() if k.endswith("rms_codes"))


def test_committed_u16_bars_are_derived():
    """tests/golden/parity_slack.json holds the 16-bit route's bars as the tool derives them: measured + margin, capped, below
    half an 8-bit hop's RMS, and never looser than the float route's max bar the route used before"""
    tool = _tool()
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "parity_slack.json")))
    bars = committed["bars"]
    for model in ("2x", "4x"):
        rms, mx = bars[f"{model}/u16/rms_codes"], bars[f"{model}/u16/max_codes"]
        assert rms["bar"] == pytest.approx(min(rms["measured_max"] + tool.MARGIN["rms_codes"], rms["cap"]))
        assert mx["bar"] == pytest.approx(min(mx["measured_max"] + tool.MARGIN["max_codes"], mx["cap"]))
        assert rms["bar"] < 257 / np.sqrt(12) / 2
        assert mx["bar"] <= 65535 * bars[f"{model}/float/f32_abs"]["bar"] + 0.1
        assert pr.slack(model, "u16", "rms_codes", None) == rms["bar"]
