"""uva_destroy_gpu_instance and what comes after it (-m gpu): every stage of the library keeps a context per device -- streams,
buffers, uploaded tables, "attribute already set" flags -- in a translation unit of its own (csrc/uva_denoise.hip, uva_png.hip,
uva_frames.hip, uva_resize.hip, and the nets of uva_api.hip with the generic executor of uva_generic_run.hip).  Each is used
once, everything is torn down, each is used again: the same bytes, and no error."""
import ctypes
import os

import numpy as np
import pytest

import generic_probe as gp
from conftest import ROOT, load_net

pytestmark = pytest.mark.gpu


def _denoise_u16(L, img, strength):
    h, w, _ = img.shape
    out = np.empty_like(img)
    rc = L.uva_denoise_u16(0, img.ctypes.data, h, w, ctypes.c_size_t(w * 6), out.ctypes.data, ctypes.c_size_t(w * 6), strength, strength)
    assert rc == 0, L.uva_last_error()
    return out


def _generic_net(uva, directory):
    """4x_Valar_v1 where its weights are on the machine, else a dense-block probe graph (u8 route) of tests/generic_probe.py"""
    param, model = (os.path.join(ROOT, "models", "4x_Valar_v1" + ext) for ext in (".param", ".bin"))
    if not os.path.exists(model):
        param, model = gp.write_probe(gp.g_dense(u8=True), 0, directory)
    net = uva.Net()
    net.set_vulkan_device(0)
    assert net.load_param(param) == 0 and net.load_model(model) == 0
    return net


def test_every_stage_gives_the_same_bytes_after_destroy_gpu_instance(uva, oracle, tmp_path):
    from upscale_video_amd import upscale_processing as up
    assert uva.get_gpu_count() > 0, "no HIP device: the HIP path cannot run (no CPU fallback exists)"
    L = uva._lib.load()
    h, w = 24, 32
    frame = oracle.synthetic_frame(h, w, seed=41)
    other = oracle.synthetic_frame(h, w, seed=42)
    frame16 = frame.astype(np.uint16) * 257 + 3
    small = gp.probe_input(16, 16, seed=5, u8=True)
    compact = load_net(uva, "2x")
    generic = _generic_net(uva, tmp_path)
    assert L.uva_net_debug_generic_plan(generic._h, (ctypes.c_int * 8)()) == 0, "the second net must run as a generic graph"

    def everything():
        return {
            "denoise_u8": up.denoise_u8(frame, 3.0, device=0),
            "denoise_u16": _denoise_u16(L, frame16, 3.0),
            "png_deflate_u8": np.frombuffer(uva.png_encode_u8(frame), np.uint8),
            "pix_convert": uva.convert_pix(frame, h, w, "bgr24", "yuv420p"),
            "resize": uva.resize(frame, (36, 20)),
            "frame_diff": np.array(uva.frame_diff(frame, other, "bgr24", h, w, threshold=2), np.uint64),
            "compact": compact.process_u8(frame),
            "generic": generic.process_u8(small),
        }

    first = everything()
    assert first["compact"].shape == (2 * h, 2 * w, 3) and first["generic"].shape[2] == 3
    assert first["frame_diff"][0] > 0, "the two frames must differ, or the comparison proves nothing"
    uva.destroy_gpu_instance()
    second = everything()
    for name in first:
        assert first[name].dtype == second[name].dtype and np.array_equal(first[name], second[name]), name
    # and a second teardown with every context rebuilt finds them all again
    uva.destroy_gpu_instance()
    assert np.array_equal(compact.process_u8(frame), first["compact"])
