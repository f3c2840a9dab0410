"""What hipcc emits for trunkw_kernel with and without the producers' carry, looked at: no GPU needed, seconds.

The carry costs 32 accumulator registers, paid from the producers' fragment queue (TW_PFF 12 -> 6).  The kernel runs two waves
per SIMD, 256 registers each, and a spill into scratch would leave it correct and slow: every instantiation must fit, and the
carry must be what it claims -- 32 instead of 48 fragment reads in the producers' k-loop for the same 96 MFMAs."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def wino_asm(tmp_path_factory):
    from upscale_video_amd import build
    asm = str(tmp_path_factory.mktemp("isa") / "uva_wino.s")
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "uva_wino.hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(asm).read()


def kernels(text):
    """mangled name -> (body, metadata block) of every trunkw_kernel instantiation"""
    out = {}
    for name in sorted(set(re.findall(r"^(_ZN3uva13trunkw_kernelILi64ELi\dELb[01]EEEvNS_10TrunkwArgsE):", text, flags=re.M))):
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index("s_endpgm")]
        at = text.index(".name:", text.index("amdhsa.kernels"))
        at = text.index(".name:           " + name, at)
        meta = text[text.rfind("- .agpr_count", 0, at):]
        out[name] = (body, meta[:meta.index(".wavefront_size")])
    return out


def test_every_instantiation_fits_256_registers_without_scratch(wino_asm):
    ks = kernels(wino_asm)
    assert len(ks) == 6, sorted(ks)              # three PReLU forms, with the carry (the product) and without (the tests' yardstick)
    for name, (body, meta) in ks.items():
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, meta).group(1))
        assert field("vgpr_spill_count") == 0 and field("private_segment_fixed_size") == 0, (name, meta)
        assert field("vgpr_count") + field("agpr_count") <= 256, (name, meta)
        assert "scratch_" not in body, name
    assert not re.search(r"ScratchSize: [1-9]", wino_asm)


def test_the_carry_reads_a_third_fewer_fragments_for_the_same_mfmas(wino_asm):
    ks = kernels(wino_asm)
    for act in "012":
        with_carry = ks["_ZN3uva13trunkw_kernelILi64ELi%sELb1EEEvNS_10TrunkwArgsE" % act][0]
        without = ks["_ZN3uva13trunkw_kernelILi64ELi%sELb0EEEvNS_10TrunkwArgsE" % act][0]
        # the two k-loops' 192 MFMAs, + the 24 that make the carried sums of a workgroup's first step from its two extra rows
        assert without.count("v_mfma_f32_16x16x32_f16") == 192 and with_carry.count("v_mfma_f32_16x16x32_f16") == 192 + 24
        # 48 -> 32 reads in the producers' k-loop, + those 16 once per launch: as many ds_read_b128 in the text, a third fewer executed
        assert with_carry.count("ds_read_b128") == without.count("ds_read_b128")
        # the producers' k-loop is the one straight run of 96 MFMAs with nothing but LDS reads between them
        runs = re.findall(r"(?:[^\n]*(?:v_mfma_f32_16x16x32_f16|ds_read_b128|s_waitcnt lgkmcnt|s_nop|sched_barrier)[^\n]*\n)+", with_carry)
        loops = [r for r in runs if r.count("v_mfma") == 96]
        assert len(loops) == 1 and loops[0].count("ds_read_b128") == 32, [(r.count("v_mfma"), r.count("ds_read_b128")) for r in runs if "v_mfma" in r]
