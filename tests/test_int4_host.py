"""The INT4 (W4A8) interchange format and quantizer as numpy states them (capi.pack_int4 / unpack_int4 / quantize_int4_host): no GPU."""
import numpy as np
import pytest

from fast_llama_amd import capi


def quantizer_inputs():
    """groups of 64: all zero | maximum negative | every multiple of max / 7 (truncation boundaries) and values just inside them | plain"""
    z, neg = np.zeros(64, np.float32), np.linspace(-3.5, 1.0, 64).astype(np.float32)
    k = np.arange(-7, 8, dtype=np.float32)
    edge = np.concatenate([k * np.float32(0.25), np.nextafter(k * np.float32(0.25), np.float32(0)), np.full(34, 1.75, np.float32)]).astype(np.float32)
    plain = np.random.default_rng(4).standard_normal(64).astype(np.float32)
    return np.concatenate([z, neg, edge, plain])


def test_pack_unpack_all_nibble_pairs_and_byte_order():
    lo, hi = np.meshgrid(np.arange(-8, 8, dtype=np.int8), np.arange(-8, 8, dtype=np.int8))
    q = np.stack([lo.ravel(), hi.ravel()], axis=1).reshape(1, -1)           # element 2i = lo, element 2i + 1 = hi
    p = capi.pack_int4(q)
    assert p.dtype == np.uint8 and p.shape == (1, 256)
    assert np.array_equal(p[0] & 0xF, lo.ravel().astype(np.uint8) & 0xF) and np.array_equal(p[0] >> 4, hi.ravel().astype(np.uint8) & 0xF)
    assert np.array_equal(capi.unpack_int4(p), q)


def test_quantize_int4_host_rule():
    x = quantizer_inputs()
    p, r = capi.quantize_int4_host(x)
    q = capi.unpack_int4(p).reshape(-1, 64)
    g = x.reshape(-1, 64)
    assert np.array_equal(r, (np.abs(g).max(axis=1) / np.float32(7)).astype(np.float32))
    assert r[0] == 0 and not q[0].any()
    assert q.min() >= -7 and q.max() <= 7 and q[1].min() == -7 and q[2].max() == 7 and q[2].min() == -7
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.trunc((g[1:] / r[1:, None]).astype(np.float32))
    assert np.array_equal(q[1:], want.astype(np.int8))
