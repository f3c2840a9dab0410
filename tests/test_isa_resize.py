"""What hipcc emits for the resampler (csrc/uva_resize.hip), looked at without a GPU: every instantiation
of resize_kernel -- u8 and u16 samples x the seven tap-count classes -- compiles for gfx950 with no scratch, stays within the
registers and the occupancy planned for its class, the u16 horizontal sums are 64-bit multiply-adds, and the LDS the host may ask
for fits the default 64 KiB (far inside the CU's 160 KiB)."""
import os
import re
import subprocess

CLASSES = (2, 4, 6, 8, 12, 16, 24)
# planned per horizontal tap-count class: 2 registers per tap (weight, LDS offset; the u16 sums twice that in flight) on top of
# pass 1's twelve loads in flight; the waves per SIMD that leaves (7: the 20 KB tiles of the common ratios fill the CU's LDS)
VGPR_CAP = {"h": {2: 64, 4: 64, 6: 64, 8: 64, 12: 64, 16: 64, 24: 80}, "t": {2: 64, 4: 64, 6: 64, 8: 64, 12: 80, 16: 112, 24: 160}}
OCC_MIN = {"h": {2: 7, 4: 7, 6: 7, 8: 7, 12: 7, 16: 7, 24: 6}, "t": {2: 7, 4: 7, 6: 7, 8: 7, 12: 6, 16: 4, 24: 3}}

def _kernels(text):
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w*resize_kernel\w+):", text, flags=re.M):
        name = m.group(1)
        seg = text[m.end():]
        seg = seg[:seg.index("; Occupancy:") + 40]
        num = lambda pat: int(re.search(pat, seg).group(1))   # noqa: E731
        info[name] = dict(scratch=num(r"; ScratchSize: (\d+)"), occ=num(r"; Occupancy: (\d+)"), vgpr=num(r"; NumVgprs: (\d+)"),
                          lds=num(r"; LDSByteSize: (\d+)"), mad64=seg.count("v_mad_i64_i32"), mad64u=seg.count("v_mad_u64_u32"))
    return info


def test_resize_kernel_resources(tmp_path):
    from upscale_video_amd import build
    asm = str(tmp_path / "resize_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_resize.hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(asm).read()
    info = _kernels(text)
    assert len(info) == 2 * len(CLASSES), sorted(info)
    addr_mads = {}
    for ty in "ht":                       # uint8_t, uint16_t in the mangled names
        for c in CLASSES:
            k = [v for name, v in info.items() if re.search(r"resize_kernelI%sLi%dEE" % (ty, c), name)]
            assert len(k) == 1, (ty, c, sorted(info))
            k = k[0]
            print("resize_kernel<%s, %d>: %d VGPRs, occupancy %d, scratch %d" % ("u8" if ty == "h" else "u16", c, k["vgpr"], k["occ"], k["scratch"]))
            assert k["scratch"] == 0 and k["lds"] == 0, (ty, c, k)          # (the tile's LDS is dynamic: sized per launch)
            assert k["vgpr"] <= VGPR_CAP[ty][c] and k["occ"] >= OCC_MIN[ty][c], (ty, c, k)
            # the u16 horizontal sums: one 64-bit multiply-add per tap (v_mad_i64_i32, or the compiler's v_mad_u64_u32 form with
            # a sign correction) on top of what the u8 twin has (address arithmetic)
            mads = k["mad64"] + k["mad64u"]
            print("    64-bit multiply-adds: %d signed, %d unsigned" % (k["mad64"], k["mad64u"]))
            if ty == "h":
                addr_mads[c] = mads
            else:
                assert mads >= addr_mads[c] + c, (ty, c, k, addr_mads)
    # the host's bound on the dynamic LDS: 16 rows of the widest footprint (64 columns at ratio 4 + 24 taps) in 32-bit words
    widest = ((64 * 4 + 24 + 1) * 3 + 6 + 3) // 4 * 4
    assert 16 * widest * 4 <= 64 * 1024 <= 160 * 1024
    src = open(os.path.join(build.CSRC, "uva_resize.hip")).read()
    assert "RS_LDS_MAX = 64 * 1024" in src and "RS_TOH = 16, RS_TOW = 64" in src
