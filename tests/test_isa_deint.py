"""What hipcc emits for the deinterlacing kernel (csrc/uva_deint.hip), looked at without a GPU: all six
instantiations -- byte samples and 16-bit words, component strides 1, 2 and 3 -- compile for gfx950 with no scratch, no LDS at
all, 16-byte global loads and stores, and few enough registers to sit beside a resident workgroup of the nets' persistent
kernels.  Only resource lines and access widths are asserted."""
import os
import re
import subprocess

VGPR_CAP = 72          # the level DESIGN.md section 7.12 records for crop_sums_kernel, rounded up to the allocation step


def _kernels(text):
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w*deint_kernel\w+):", text, flags=re.M):
        name = m.group(1)
        seg = text[m.end():]
        seg = seg[:seg.index("; Occupancy:") + 40]
        num = lambda pat: int(re.search(pat, seg).group(1))   # noqa: E731
        info[name] = dict(scratch=num(r"; ScratchSize: (\d+)"), occ=num(r"; Occupancy: (\d+)"), vgpr=num(r"; NumVgprs: (\d+)"),
                          lds=num(r"; LDSByteSize: (\d+)"), load_x4=seg.count("global_load_dwordx4"),
                          store_x4=seg.count("global_store_dwordx4"))
    return info


def test_deint_kernel_resources(tmp_path):
    from upscale_video_amd import build
    asm = str(tmp_path / "deint_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_deint.hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    info = _kernels(open(asm).read())
    assert len(info) == 6, sorted(info)
    for nbytes in (1, 2):
        for stride in (1, 2, 3):
            k = [v for name, v in info.items() if re.search(r"deint_kernelILi%dELi%dEE" % (nbytes, stride), name)]
            assert len(k) == 1, (nbytes, stride, sorted(info))
            k = k[0]
            print("deint_kernel<%d, %d>: %d VGPRs, occupancy %d, scratch %d, LDS %d, %d 16-byte loads, %d 16-byte stores" %
                  (nbytes, stride, k["vgpr"], k["occ"], k["scratch"], k["lds"], k["load_x4"], k["store_x4"]))
            assert k["scratch"] == 0, k
            assert k["lds"] == 0, k                                  # no static LDS either; the launch asks for no dynamic LDS
            assert k["vgpr"] <= VGPR_CAP, k
            # the kept row's copy and the rows of the rule; the copy's store and the interpolated unit's
            assert k["load_x4"] >= 13 and k["store_x4"] >= 2, k
    src = open(os.path.join(build.CSRC, "uva_deint.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(\(deint_kernel<B, S>\), dim3\(groups\), dim3\(DI_THREADS\), 0, stream", src)
    assert "extern __shared__" not in src and "__shared__" not in src
