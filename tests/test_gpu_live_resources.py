"""Every HIP buffer, stream and event of the library is held by a handle (csrc/uva_own.h) and the handles are counted:
uva_debug_live_resources (-m gpu).  The counters say whether the teardown paths -- load_model on a used net, uva_deint_destroy,
uva_net_destroy, uva_destroy_gpu_instance -- give back everything, and a process that exits with everything still alive must
exit cleanly: no static destructor calls the runtime.

"Zero before any use" can only be seen in a process that has not used the library yet, so the scenario runs in a fresh child
(this file as a program: `scenario`, `exit-plain`, `exit-teardown`) and reports what it saw as one JSON line."""
import ctypes
import gc
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

KINDS = ("device buffers", "host buffers", "streams", "events")


def _live(L):
    c = (ctypes.c_longlong * 4)()
    L.uva_debug_live_resources(c)
    return list(c)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _use_everything(uva, oracle, gp, load_net, directory, report):
    """every owner once on tiny frames -> {name: hash of the bytes}; the nets and the deinterlacer are gone when it returns"""
    from upscale_video_amd import upscale_processing as up
    L = uva._lib.load()
    h, w = 24, 32
    frame = oracle.synthetic_frame(h, w, seed=41)
    other = oracle.synthetic_frame(h, w, seed=42)
    frame16 = frame.astype(np.uint16) * 257 + 3
    small = gp.probe_input(16, 16, seed=5, u8=True)
    small1 = oracle.synthetic_frame(16, 16, seed=43)
    out = {}
    two = load_net(uva, "2x")
    out["process_u8"] = _sha(two.process_u8(frame))
    # the pipelined route: three frames in flight, the second repeats the first
    two.set_skip_repeats(0)
    tickets = [two.submit_u8(f) for f in (frame, frame, other)]
    got = [two.collect_u8(t).copy() for t in tickets]
    assert two.skip_stats() == (3, 1) and np.array_equal(got[0], got[1])
    out["pipelined"] = _sha(np.stack(got))
    two.set_skip_repeats(None)
    yuv = uva.convert_pix(frame, h, w, "bgr24", "yuv420p")
    out["convert_pix"] = _sha(yuv)
    out["submit_pix"] = _sha(two.collect_u8(two.submit_pix(yuv, h, w, "yuv420p", out_fmt="yuv420p")))
    out["submit_png"] = _sha(np.frombuffer(two.collect_u8(two.submit_u8_png(frame)).file_bytes(), np.uint8))
    out["process_u16"] = _sha(two.process_u16(frame16))
    out["denoise_u8"] = _sha(up.denoise_u8(frame, 3.0, device=0))
    d16 = np.empty_like(frame16)
    assert L.uva_denoise_u16(0, frame16.ctypes.data, h, w, ctypes.c_size_t(w * 6), d16.ctypes.data, ctypes.c_size_t(w * 6),
                             ctypes.c_float(3.0), ctypes.c_float(3.0)) == 0, L.uva_last_error()
    out["denoise_u16"] = _sha(d16)
    out["resize"] = _sha(uva.resize(frame, (36, 20)))
    out["frame_diff"] = _sha(np.array(uva.frame_diff(frame, other, "bgr24", h, w, threshold=2), np.uint64))
    di = uva.Deinterlacer("yuv420p", h, w)
    outs = [np.empty(di.nbytes, np.uint8)]
    assert di.push(yuv, outs) == 0 and di.push(yuv[::-1].copy(), outs) == 1
    out["deint"] = _sha(outs[0])
    param, model = gp.write_probe(gp.g_dense(u8=True), 0, directory)
    gen = uva.Net()
    gen.set_vulkan_device(0)
    assert gen.load_param(param) == 0 and gen.load_model(model) == 0
    out["generic"] = _sha(gen.process_u8(small))
    # load_model on a used net gives back all that the net took when it first ran
    one = load_net(uva, "1x")
    before = _live(L)
    out["1x"] = _sha(one.process_u8(small1))
    report["net_took"] = [a - b for a, b in zip(_live(L), before)]
    from conftest import model_paths
    assert one.load_model(model_paths("1x")[1]) == 0
    report["after_load_model"] = [a - b for a, b in zip(_live(L), before)]
    report.setdefault("in_use", []).append(_live(L))
    di.close()
    del two, one, gen, tickets
    gc.collect()
    uva.destroy_gpu_instance()
    report.setdefault("after_teardown", []).append(_live(L))
    return out


def _child(mode):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["UVA_DEBUG_SWITCHES"] = "1"
    import generic_probe as gp
    from conftest import load_net
    from oracle import uvoracle
    from upscale_video_amd import ncnn as uva
    L = uva._lib.load()
    report = {"before_any_use": _live(L)}
    with tempfile.TemporaryDirectory() as tmp:
        if mode == "scenario":
            first = _use_everything(uva, uvoracle, gp, load_net, tmp, report)
            second = _use_everything(uva, uvoracle, gp, load_net, tmp, report)
            report["bytes"] = [first, second]
        else:
            # every stage once, everything still alive when the interpreter goes: a net, a deinterlacer, every stage's context
            frame = uvoracle.synthetic_frame(24, 32, seed=41)
            keep = [load_net(uva, "2x"), uva.Deinterlacer("yuv420p", 24, 32)]
            keep[0].process_u8(frame)
            from upscale_video_amd import upscale_processing as up
            up.denoise_u8(frame, 3.0, device=0)
            uva.png_encode_u8(frame)
            uva.convert_pix(frame, 24, 32, "bgr24", "yuv420p")
            uva.resize(frame, (36, 20))
            report["in_use"] = [_live(L)]
            if mode == "exit-teardown":
                uva.destroy_gpu_instance()
                report["after_teardown"] = [_live(L)]
            # the net and the deinterlacer are never destroyed, not even by the interpreter on its way out: what is tested is
            # the exit of a process in which the library still holds them
            uva.Net.__del__ = lambda self: None
            uva.Deinterlacer.__del__ = lambda self: None
    print(json.dumps(report), flush=True)


def _run_child(mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, "%s: exit status %d\n%s" % (mode, r.returncode, (r.stdout + r.stderr)[-4000:])
    for word in ("hip", "HIP", "HSA", "rocm", "Aborted", "Segmentation", "terminate", "core dumped"):
        assert word not in r.stderr, "%s: the child's stderr mentions %r:\n%s" % (mode, word, r.stderr[-4000:])
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_every_resource_is_counted_and_every_teardown_gives_all_of_them_back():
    rep = _run_child("scenario")
    print(json.dumps(rep))
    assert rep["before_any_use"] == [0, 0, 0, 0]
    for use in rep["in_use"]:
        assert all(v > 0 for v in use), dict(zip(KINDS, use))
    # the 1x net took device buffers and a stream of its own when it first ran, and load_model gave back exactly those
    assert rep["net_took"][0] > 0 and rep["net_took"][2] > 0, rep["net_took"]
    assert rep["after_load_model"] == [0, 0, 0, 0]
    assert rep["after_teardown"] == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert rep["bytes"][0] == rep["bytes"][1] and len(rep["bytes"][0]) == 13


@pytest.mark.parametrize("mode", ["exit-plain", "exit-teardown"])
def test_a_process_that_exits_with_everything_alive_exits_cleanly(mode):
    rep = _run_child(mode)
    assert rep["before_any_use"] == [0, 0, 0, 0] and all(v > 0 for v in rep["in_use"][0][:3])
    if mode == "exit-teardown":
        # the net's state went with uva_destroy_gpu_instance; the deinterlacer is its caller's: three frames, one output, a stream
        assert rep["after_teardown"] == [[4, 0, 1, 0]]


if __name__ == "__main__":
    _child(sys.argv[1])
