"""What hipcc emits for the inverse telecine's metric kernel (csrc/uva_ivtc.hip), looked at without a GPU:
both instantiations -- byte samples and 16-bit words -- compile for gfx950 with no scratch, no floating point, a few words of
static LDS for the reduction, 16-byte global loads, and few enough registers to sit beside a resident workgroup of the nets'
persistent kernels.  Only resource lines and instruction names are asserted."""
import os
import re
import subprocess

VGPR_CAP = 72          # the deinterlacing kernel's budget (tests/test_isa_deint.py); the compiler gives 69 and 71


def _kernels(text):
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w*ivtc_metrics_kernel\w+):", text, flags=re.M):
        name = m.group(1)
        seg = text[m.end():]
        seg = seg[:seg.index("; Occupancy:") + 40]
        num = lambda pat: int(re.search(pat, seg).group(1))   # noqa: E731
        info[name] = dict(scratch=num(r"; ScratchSize: (\d+)"), occ=num(r"; Occupancy: (\d+)"), vgpr=num(r"; NumVgprs: (\d+)"),
                          lds=num(r"; LDSByteSize: (\d+)"), load_x4=seg.count("global_load_dwordx4"),
                          floats=len(re.findall(r"\bv_(?:cvt_f|rcp_|mul_f|add_f|fma_f|mac_f)", seg)),
                          atomics=seg.count("global_atomic_add_x2"))
    return info


def test_ivtc_kernel_resources(tmp_path):
    from upscale_video_amd import build
    asm = str(tmp_path / "ivtc_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_ivtc.hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    info = _kernels(open(asm).read())
    assert len(info) == 2, sorted(info)
    for nbytes in (1, 2):
        k = [v for name, v in info.items() if re.search(r"ivtc_metrics_kernelILi%dEE" % nbytes, name)]
        assert len(k) == 1, (nbytes, sorted(info))
        k = k[0]
        print("ivtc_metrics_kernel<%d>: %d VGPRs, occupancy %d, scratch %d, LDS %d, %d 16-byte loads, %d float instructions" %
              (nbytes, k["vgpr"], k["occ"], k["scratch"], k["lds"], k["load_x4"], k["floats"]))
        assert k["scratch"] == 0, k
        assert k["vgpr"] <= VGPR_CAP, k
        assert k["lds"] == 4 * 6 * 8, k                          # the four waves' six sums; the launch asks for no dynamic LDS
        assert k["floats"] == 0, k
        assert k["load_x4"] >= 4, k                              # whole slots are 16-byte loads
        assert k["atomics"] == 1, k                              # one set of 64-bit adds per workgroup (six lanes of one instruction)
    src = open(os.path.join(build.CSRC, "uva_ivtc.hip")).read()
    # the launch goes to the caller's stream, and csrc/uva_frames.hip hands it the handle's
    assert len(re.findall(r"hipLaunchKernelGGL\(ivtc_metrics_kernel<[12]>, groups, dim3\(IV_THREADS\), 0, stream, a\)", src)) == 2
    assert re.search(r"hipMemsetAsync\(d_stats, 0, 6 \* sizeof\(unsigned long long\), stream\)", src)
    assert "extern __shared__" not in src
    frames = open(os.path.join(build.CSRC, "uva_frames.hip")).read()
    assert "launch_ivtc_metrics(d->stream, prev, cur, next, d->fmt, d->h, d->w, d->flags, d->T, d->d_stats, 0)" in frames
    assert "launch_ivtc_weave(d->stream," in frames and "launch_frame_diff(d->stream, dst," in frames
    assert re.search(r"launch_deint\(d->stream, prev, cur, next, d->fmt, d->h, d->w, ivtc_deint_flags\(d->flags\), dst, nullptr, 0\)", frames)
