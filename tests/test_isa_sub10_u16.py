"""What hipcc emits for sub10_kernel16, looked at without a GPU, from the resource comments of its
assembly alone: no scratch, registers for the three waves per SIMD that a 768-thread workgroup needs, the LDS the launcher asks
for within a CU's 160 KiB -- and sub10_kernel beside it still without scratch."""
import re
import subprocess

TU = r"""
#include "uva_sub10.hip.h"
namespace uva {
static_assert(sub10_lds_bytes16() <= 160 * 1024, "sub10 u16 LDS budget");
static_assert(sub10_lds_bytes16() == sub10_lds_bytes() - S10_RESB, "the u16 kernel keeps no residual ring");
static_assert(sub10_lds_bytes() <= 160 * 1024, "sub10 LDS budget");
}
"""


def _kernels(text):
    """kernel symbol -> (scratch bytes, occupancy in waves per SIMD, VGPRs + AGPRs) from hipcc's assembly comments"""
    info = {}
    for m in re.finditer(r"^(_ZN3uva\w+):", text, flags=re.M):
        name = m.group(1)
        tail = text[m.end():]
        end = tail.find(".size\t" + name) if (".size\t" + name) in tail else len(tail)
        seg = tail[:end + 4000]
        if not re.search(r"; ScratchSize: (\d+)", seg):
            continue
        scratch = int(re.search(r"; ScratchSize: (\d+)", seg).group(1))
        occ = int(re.search(r"; Occupancy: (\d+)", seg).group(1))
        regs = int(re.search(r"; NumVgprs: (\d+)", seg).group(1)) + int(re.search(r"; NumAgprs: (\d+)", seg).group(1))
        info[name] = (scratch, occ, regs)
    return info


def test_sub10_kernel16_resources(tmp_path):
    from upscale_video_amd import build
    src = tmp_path / "sub10_u16_isa.hip"
    src.write_text(TU)
    asm = str(tmp_path / "sub10_u16_isa.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-I", build.CSRC, "-S", "--cuda-device-only", str(src), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    info = _kernels(open(asm).read())
    k8 = [v for k, v in info.items() if re.search(r"12sub10_kernelE", k)]
    k16 = [v for k, v in info.items() if re.search(r"14sub10_kernel16E", k)]
    assert len(k8) == 1 and len(k16) == 1, info
    assert k8[0][0] == 0, info                  # sub10_kernel: still no scratch
    scratch, occ, regs = k16[0]
    assert scratch == 0, info
    # 12 waves on 4 SIMDs: three per SIMD, 512 registers each -> at most 168 per wave (allocated in blocks of 8)
    assert occ >= 3 and regs <= 168, info
