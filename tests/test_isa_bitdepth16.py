"""What hipcc emits for the 16-bit route's kernels, looked at without a GPU: the u16 head and tails
compile for gfx950 with no scratch, the LDS the host reserves for them, and the occupancy of their u8 twins."""
import os
import re
import subprocess

TU = r"""
#include "uva_kernels.hip.h"
namespace uva {
template __global__ void headp_kernel<64, 0>(HeadArgs);
template __global__ void headp_kernel<64, 2>(HeadArgs);
template __global__ void tail_kernel<64, 2, uint8_t>(ConvArgs);
template __global__ void tail_kernel<64, 2, uint16_t>(ConvArgs);
template __global__ void tail4_kernel<64, uint8_t>(ConvArgs);
template __global__ void tail4_kernel<64, uint16_t>(ConvArgs);
// the planned LDS: the u16 tails need twice the residual area (8 waves x 256 B) and still fit the CU's 160 KiB
static_assert(tail_lds_bytes<64, uint16_t>() == tail_lds_bytes<64>() + 1024, "tail LDS");
static_assert(tail4_lds_bytes<64, uint16_t>() == tail4_lds_bytes<64>() + 1024, "tail4 LDS");
static_assert(tail_lds_bytes<64, uint16_t>() <= 160 * 1024 && tail4_lds_bytes<64, uint16_t>() <= 160 * 1024, "LDS budget");
}
"""


def _kernels(text):
    """kernel symbol -> (scratch bytes, occupancy in waves per SIMD, VGPRs) from hipcc's assembly comments"""
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w+):", text, flags=re.M):
        name = m.group(1)
        tail = text[m.end():]
        end = tail.find(".size\t" + name) if (".size\t" + name) in tail else len(tail)
        seg = tail[:end + 4000]
        scratch = int(re.search(r"; ScratchSize: (\d+)", seg).group(1))
        occ = int(re.search(r"; Occupancy: (\d+)", seg).group(1))
        vgpr = int(re.search(r"; NumVgprs: (\d+)", seg).group(1))
        info[name] = (scratch, occ, vgpr)
    return info


def test_u16_head_and_tails_keep_the_u8_occupancy(tmp_path):
    from upscale_video_amd import build
    src = tmp_path / "bd16_isa.hip"
    src.write_text(TU)
    asm = str(tmp_path / "bd16_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-I", build.CSRC, "-S", "--cuda-device-only", str(src), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    info = _kernels(open(asm).read())
    pick = lambda pat: [v for k, v in info.items() if re.search(pat, k)]   # noqa: E731
    head8, head16 = pick(r"headp_kernelILi64ELi0E"), pick(r"headp_kernelILi64ELi2E")
    tail8, tail16 = pick(r"tail_kernelILi64ELi2EhE"), pick(r"tail_kernelILi64ELi2EtE")
    t48, t416 = pick(r"tail4_kernelILi64EhE"), pick(r"tail4_kernelILi64EtE")
    assert all(len(x) == 1 for x in (head8, head16, tail8, tail16, t48, t416)), info
    for (s8, o8, _), (s16, o16, v16) in ((head8[0], head16[0]), (tail8[0], tail16[0]), (t48[0], t416[0])):
        assert s16 == 0 and s8 == 0, info
        assert o16 == o8, info          # the same waves per SIMD as the u8 twin
    assert tail16[0][1] >= 2 and t416[0][1] >= 2, info     # 8-wave workgroups: two waves per SIMD
