"""CPU emulation of the six-term bf16 product whose BOTH operands are split in registers (children_fused_kernel, BX mode:
the crowd's S = G Xh^T and U = E Xh, the tile's robot row / column of S -- b6_block in rgl_fused_kernel.hip).

Each operand element x is split by round-to-nearest-even into bf16 pieces h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)
(split3_pair); the block sums the six terms l.h, m.m, h.l, m.h, h.m, h.h (weight piece first), each one K = 32 MFMA whose
bf16 x bf16 products are exact in f32 and are added into an f32 accumulator.  The dropped terms (m.l, l.m, l.l) are below
2^-25 of |a||b|, so the block's error stays within 2^-23 sum |a||b| -- the bound the six-term layers already meet.
"""
import numpy as np
import pytest


def bf16_rn(x):
    """float32 -> nearest-even bfloat16, returned as float32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rn(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_rn(r1)
    lo = bf16_rn((r1 - m).astype(np.float32))
    return h, m, lo


def b6_block(a, b):
    """a [16][32], b [32][16] float32 -> a b over the six terms, f32 accumulation term by term in the kernel's order"""
    ah, am, al = split3(a)
    bh, bm, bl = split3(b)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for pa, pb in ((al, bh), (am, bm), (ah, bl), (am, bh), (ah, bm), (ah, bh)):
        prod = pa.astype(np.float64)[:, :, None] * pb.astype(np.float64)[None, :, :]    # exact: 8 x 8 significant bits
        for k in range(a.shape[1]):
            acc = (acc + prod[:, k, :].astype(np.float32)).astype(np.float32)
    return acc


def check(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    want = a.astype(np.float64) @ b.astype(np.float64)
    got = b6_block(a, b).astype(np.float64)
    bound = 2.0 ** -23 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))
    err = np.abs(got - want)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


def test_split3_is_exact():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4096), rng.uniform(-1e6, 1e6, 1024), rng.uniform(0, 1e-20, 256)]).astype(np.float32)
    h, m, lo = split3(x)
    assert np.array_equal((h.astype(np.float64) + m + lo).astype(np.float32), x)
    for p in (h, m, lo):
        assert np.array_equal(p, bf16_rn(p))


@pytest.mark.parametrize("seed", range(4))
def test_b6_block_random(seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((16, 32)) * rng.choice([1e-3, 1.0, 30.0], size=(16, 1))
    b = rng.standard_normal((32, 16))
    check(a, b)


def test_b6_block_attention_logits():
    # the crowd / robot S products: G = Xh Wa rows against ReLU features, logits in the hundreds
    rng = np.random.default_rng(7)
    xh = np.maximum(rng.standard_normal((16, 32)) * 4.0, 0.0)
    g = rng.standard_normal((32, 16)) * 6.0
    check(xh, g)


def test_b6_block_adversarial():
    rng = np.random.default_rng(11)
    # cancellation: b's columns nearly orthogonal to a's rows; elements next to bf16 rounding ties; mixed magnitudes
    a = rng.standard_normal((16, 32)).astype(np.float32)
    b = rng.standard_normal((32, 16)).astype(np.float32)
    b[:, 0] = a[0] * np.float32(1.0)
    b[16:, 0] = -a[0, :16]
    ties = (1.0 + (2.0 ** -8) * (np.arange(32) % 2) + 2.0 ** -9).astype(np.float32)      # halfway between bf16 neighbours
    a[1] = ties
    b[:, 1] = ties[::-1]
    a[2] = np.float32(1e30) * rng.standard_normal(32).astype(np.float32)
    b[:, 2] = np.float32(1e-30) * rng.standard_normal(32).astype(np.float32)
    a[3, ::2] = 3.0e4
    a[3, 1::2] = -3.0e4
    b[:, 3] = 1.0 + 2.0 ** -20 * np.arange(32)
    check(a, b)
