"""What hipcc emits for the frame-difference kernel (csrc/uva_repeat.hip), looked at without a GPU: both
instantiations -- byte samples and 16-bit words -- compile for gfx950 with no scratch, walk the frames with 16-byte global loads,
reach the narrow loads only for the last partial unit, and stay small enough (registers, a few dozen bytes of static LDS, no dynamic
LDS) to sit beside a resident workgroup of the nets' persistent kernels."""
import os
import re
import subprocess

VGPR_CAP = 32          # at 32 VGPRs a wave of this kernel fits wherever a SIMD has any room left for one
LDS_CAP = 256          # "a few hundred bytes": four waves' partial results


def _kernels(text):
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w*frame_diff_kernel\w+):", text, flags=re.M):
        name = m.group(1)
        seg = text[m.end():]
        seg = seg[:seg.index("; Occupancy:") + 40]
        num = lambda pat: int(re.search(pat, seg).group(1))   # noqa: E731
        info[name] = dict(scratch=num(r"; ScratchSize: (\d+)"), occ=num(r"; Occupancy: (\d+)"), vgpr=num(r"; NumVgprs: (\d+)"),
                          lds=num(r"; LDSByteSize: (\d+)"), x4=seg.count("global_load_dwordx4"), narrow8=seg.count("global_load_ubyte"),
                          narrow16=seg.count("global_load_ushort"), atomics=len(re.findall(r"global_atomic_\w+", seg)),
                          sad=seg.count("v_sad_u8"))
    return info


def test_frame_diff_kernel_resources(tmp_path):
    from upscale_video_amd import build
    asm = str(tmp_path / "repeat_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_repeat.hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    info = _kernels(open(asm).read())
    assert len(info) == 2, sorted(info)
    for bytes_per_sample in (1, 2):
        k = [v for name, v in info.items() if re.search(r"frame_diff_kernelILi%dEE" % bytes_per_sample, name)]
        assert len(k) == 1, (bytes_per_sample, sorted(info))
        k = k[0]
        print("frame_diff_kernel<%d>: %d VGPRs, occupancy %d, scratch %d, LDS %d, %d 16-byte loads" %
              (bytes_per_sample, k["vgpr"], k["occ"], k["scratch"], k["lds"], k["x4"]))
        assert k["scratch"] == 0, k
        assert k["x4"] >= 2, k                                   # one 16-byte load per frame and lane in the loop
        assert k["vgpr"] <= VGPR_CAP and k["occ"] == 8, k
        assert 0 < k["lds"] <= LDS_CAP, k                        # static alone; the launch asks for no dynamic LDS
        assert k["atomics"] >= 3, k                              # one set per workgroup: over, max_abs, sad
        # the last partial unit goes sample by sample, with loads of the sample's own width
        assert (k["narrow8"] >= 2 and k["narrow16"] == 0) if bytes_per_sample == 1 else (k["narrow16"] >= 2 and k["narrow8"] == 0), k
    assert [v for n, v in info.items() if "ILi1EE" in n][0]["sad"] >= 4      # bytes: v_sad_u8 sums four differences at once
    src = open(os.path.join(build.CSRC, "uva_repeat.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(frame_diff_kernel<1>, dim3\(groups\), dim3\(FD_THREADS\), 0, stream", src)
    assert re.search(r"hipLaunchKernelGGL\(frame_diff_kernel<2>, dim3\(groups\), dim3\(FD_THREADS\), 0, stream", src)
