"""The references of tests/gemm_refs.py against independent anchors (CPU, no library):
the published splitmix64 vectors, hand-computed thresholds, and the geometry of carve()."""
from __future__ import annotations

import numpy as np
import torch

import gemm_refs as R

# splitmix64 seeded with 1234567: the first five outputs of the public-domain reference
# implementation (the test vectors most ports of the generator quote)
SPLITMIX_1234567 = [6457827717110365317, 3203168211198807973, 9817491932198370423,
                    4593380528125082431, 16408922859458223821]
HIGH_WORDS = [1503580183, 745795716, 2285812965, 1069479744, 3820500071]


def test_hash_matches_published_splitmix64():
    out = R.splitmix64(1234567, np.arange(5))
    assert [int(v) for v in out] == SPLITMIX_1234567
    assert [int(v) for v in R.hash_u32(1234567, np.arange(5))] == HIGH_WORDS
    assert [v >> 32 for v in SPLITMIX_1234567] == HIGH_WORDS
    # scalar counters, and a counter at the top of the uint64 range wraps (ctr + 1 == 0)
    assert int(R.hash_u32(1234567, 3)) == HIGH_WORDS[3]
    assert int(R.splitmix64(1234567 - 0x9E3779B97F4A7C15, 1)) == SPLITMIX_1234567[0]
    assert int(R.splitmix64(0, R.MASK64)) == 0  # state 0 finalises to 0


def test_threshold_and_scale_are_the_hosts():
    assert R.drop_threshold(0.0) == 0
    assert R.drop_threshold(0.5) == 1 << 31
    assert R.drop_threshold(0.2) == 858993472  # float32(0.2) * 2^32, exactly
    assert int(0.2 * 2 ** 32) == 858993459     # what double 0.2 would have given
    assert R.drop_threshold(np.nextafter(np.float32(1), np.float32(0))) == 4294967040
    assert R.drop_scale(0.0) == np.float32(1) and R.drop_scale(0.5) == np.float32(2)
    assert R.drop_scale(0.2) == np.float32(1.25)


def test_dropout_keep_counter():
    M, N = 7, 11
    k0 = R.dropout_keep(M, N, 0.5, 123, 0)
    assert k0.shape == (M, N) and k0.dtype == np.bool_
    # the counter is offset + m*N + n: shifting the offset by one row shifts the mask by one
    kN = R.dropout_keep(M, N, 0.5, 123, N)
    assert np.array_equal(kN[:-1], k0[1:])
    k1 = R.dropout_keep(M, N, 0.5, 123, 1)
    assert np.array_equal(k1.reshape(-1)[:-1], k0.reshape(-1)[1:])
    # step s is the stream at offset s << 32; the sum wraps mod 2^64
    assert np.array_equal(R.dropout_keep(M, N, 0.5, 123, 5, step=3),
                          R.dropout_keep(M, N, 0.5, 123, 5 + (3 << 32)))
    assert np.array_equal(R.dropout_keep(M, N, 0.5, 123, 2 ** 63, step=2 ** 31),
                          R.dropout_keep(M, N, 0.5, 123, 0))
    assert not np.array_equal(R.dropout_keep(M, N, 0.5, 123, 0, step=1), k0)
    # element by element against the scalar definition
    for (m, n) in ((0, 0), (3, 4), (6, 10)):
        h = int(R.hash_u32(2 ** 64 - 1, (2 ** 64 - 5 + m * N + n) % 2 ** 64))
        assert R.dropout_keep(M, N, 0.2, 2 ** 64 - 1, 2 ** 64 - 5)[m, n] == (h >= 858993472)
    assert R.dropout_keep(M, N, 0.0, 9, 9).all()
    big = R.dropout_keep(300, 300, 0.2, 1, 0)
    assert abs(big.mean() - 0.8) < 0.01


def test_epilogue_ref():
    acc = np.array([[-2.0, 0.0, 3.0], [16777217.0, -1.0, 5.0]])  # 2^24 + 1 rounds to fp32
    bias = np.array([1.0, -1.0, 0.5], dtype=np.float32)
    out = R.epilogue_ref(acc, R.EPI_NONE)
    assert out.dtype == np.float32 and out[1, 0] == np.float32(16777216.0)
    assert np.array_equal(R.epilogue_ref(acc, R.EPI_BIAS, bias=bias),
                          np.array([[-1, -1, 3.5], [16777216, -2, 5.5]], dtype=np.float32))
    assert np.array_equal(R.epilogue_ref(acc, R.EPI_BIAS_RELU, bias=bias),
                          np.array([[0, 0, 3.5], [16777216, 0, 5.5]], dtype=np.float32))
    keep = np.array([[True, True, False], [True, True, True]])
    assert np.array_equal(
        R.epilogue_ref(acc, R.EPI_BIAS_RELU_DROP, bias=bias, keep=keep, drop_scale=1.25),
        np.array([[0, 0, 0], [20971520, 0, 6.875]], dtype=np.float32))
    aux = np.array([[1.0, -0.0, 0.0], [np.inf, -1.0, 1.0]], dtype=np.float32)
    assert np.array_equal(R.epilogue_ref(acc, R.EPI_GRAD_MASK, aux=aux, scale=1.25),
                          np.array([[-2.5, 0, 0], [20971520, 0, 6.25]], dtype=np.float32))


def test_carve_geometry():
    dev = torch.device("cpu")
    for (rows, cols, ld, off) in ((5, 7, 7, 0), (5, 7, 8, 1), (1, 3, 11, 3), (36, 40, 44, 1),
                                  (0, 4, 4, 0), (4, 0, 2, 0)):
        s = R.carve(rows, cols, ld, off, dev)
        assert tuple(s.view.shape) == (rows, cols)
        assert int(s.mask.sum()) == rows * cols
        assert s.buf.isnan().all() and s.pad_intact()
        if rows * cols == 0:
            continue
        assert s.view.stride() == (ld, 1) or rows == 1
        first = (s.view.data_ptr() - s.buf.data_ptr()) // 4
        assert first == R.HEAD + off
        last = first + (rows - 1) * ld + cols - 1
        assert s.buf.numel() - 1 - last >= 64 * ld + 64  # the margin after the last element
        idx = torch.nonzero(s.mask).reshape(-1)
        assert int(idx[0]) == first and int(idx[-1]) == last
        r, c = (idx - first) // ld, (idx - first) % ld
        assert int(c.max()) == cols - 1 and int(r.max()) == rows - 1
        assert (s.view.data_ptr() % 16 == 0) == (off % 4 == 0)
    vals = torch.arange(12.0).view(3, 4)
    o = R.carve(3, 4, 6, 1, dev, fill=R.SENTINEL, values=vals)
    assert torch.equal(o.view, vals) and o.pad_intact()
    assert torch.equal(o.buf[o.mask], vals.reshape(-1))
    o.buf[R.HEAD + 1 + 4] = 0.0  # a store into the first row's pad column
    assert not o.pad_intact()
    o.buf[R.HEAD + 1 + 4] = R.SENTINEL
    o.buf[R.HEAD] = 1.0          # ... and into the margin in front
    assert not o.pad_intact()
