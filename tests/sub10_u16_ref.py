"""numpy restatement of what sub10_kernel16 -- the 1x net on u16 BGR frames, DESIGN.md section 7.9 -- does where a pixel is
stored: the head's operand, the tail's residual and the tail's rounding, each in the kernel's own precision and order, and
their u8 twins (sub10_kernel) for comparison.  Between the two ends the kernel is sub10_kernel's trunk, which the
product-mode oracle stands for (product_u16)."""
import numpy as np

F32 = np.float32
NORM = F32(1 / 255.0)            # the kernels' `norm`: the double 1/255 rounded to fp32
INV257 = F32(1 / 257.0)


def head_operand_u16(v):
    """u16 codes -> the fp16 operand the head feeds the MFMA: fp16(v * (1/257)), the product formed in fp32"""
    return np.float16(np.asarray(v).astype(F32) * INV257)


def head_operand_u8(k):
    """u8 codes -> sub10_kernel's operand: the code itself as fp16"""
    return np.float16(np.asarray(k).astype(F32))


def head_input(v):
    """the net's input as the head's arithmetic has it: the fp16 operand times the accumulator's 1/255, float32"""
    return head_operand_u16(v).astype(F32) / F32(255.0)


def residual_u16(v):
    """u16 codes -> the residual the tail adds: ((float)v / 257.0f) * (1/255), a true fp32 division, then the fp32 product"""
    return (np.asarray(v).astype(F32) / F32(257.0)) * NORM


def residual_u8(k):
    """u8 codes -> sub10_kernel's residual: (float)k * (1/255)"""
    return np.asarray(k).astype(F32) * NORM


def tail_round_u16(y):
    """clamp(rint(y * 65535), 0, 65535) on fp32 (rint: half to even)"""
    return np.clip(np.rint(np.asarray(y, F32) * F32(65535.0)), 0, 65535).astype(np.uint16)


def tail_round_u8(y):
    """v_cvt_pk_u8_f32(y * 255): rint half to even, saturated"""
    return np.clip(np.rint(np.asarray(y, F32) * F32(255.0)), 0, 255).astype(np.uint8)


def product_u16(om, oracle, x16):
    """The product-mode oracle as the route computes a whole frame -> u16 [h][w][3]: the net's body from
    om.forward(..., product_flags()) on the head's operand, minus that input (the 1x net ends in conv + input, so the oracle's
    own residual comes off to fp32 rounding), plus the tail's own residual, and the tail's rounding."""
    xh = head_input(x16)
    raw = om.forward(np.ascontiguousarray(xh.transpose(2, 0, 1)), flags=oracle.product_flags()).transpose(1, 2, 0)
    body = raw.astype(np.float64) - xh
    return tail_round_u16(body.astype(F32) + residual_u16(x16))


def fp32_raw(om, x16):
    """the fp32 oracle on x16 / 65535 -> float32 [h][w][3], unclamped"""
    x = np.asarray(x16).astype(F32) / F32(65535.0)
    return om.forward(np.ascontiguousarray(x.transpose(2, 0, 1)), flags=0).transpose(1, 2, 0)
