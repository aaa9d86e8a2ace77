"""Batch ingestion, CPU side: oracle/ingest_oracle.py against the fixture the REAL `VidDataset` generated
(tests/golden/ingest.pt), bit for bit; and the g++ build of the kernel's own arithmetic header (csrc/ingest_math.hpp) against both."""
import os

import numpy as np
import pytest
import torch

import host_twin
from oracle import ingest_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ingest.pt")


@pytest.fixture(scope="module")
def gold():
    g = torch.load(GOLD, weights_only=False)
    m = g["meta"]
    return g, IO.synthetic_video(m["seed"], T=m["T"], H=m["H"], W=m["W"])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a, b.view(np.uint8) if b.dtype.kind == "f" else b)


def test_read_raw_matches_the_reference_bit_for_bit(gold):
    g, video = gold
    for case in g["read_raw"]:
        ours = IO.read_raw(video, case["im0idx"], case["delta"], case["xy"].numpy(), dataid=3)
        for k, ref in case["out"].items():
            assert same(np.asarray(ours[k]), ref.numpy()), (k, case["im0idx"], case["delta"])


def test_load_data_pair_stacking_and_pixel_index_arithmetic(gold):
    g, video = gold
    N, H = g["meta"]["N"], g["meta"]["H"]
    for case in g["load_data"]:
        ref = case["out"]
        q = case["queue_head"].numpy()
        xy0, xy1 = IO.sample_xy_from_idx(q[:N], H), IO.sample_xy_from_idx(q[N: 2 * N], H)
        assert np.array_equal(ref["hxy"].numpy()[0, :, :2], xy0) and np.array_equal(ref["hxy"].numpy()[1, :, :2], xy1)
        delta = int(ref["frameid_sub"][1] - ref["frameid_sub"][0])  # the delta numpy's RNG drew
        ours = IO.load_pair(video, case["im0idx"], delta, xy0, xy1, dataid=3)
        for k, r in ref.items():
            assert same(np.asarray(ours[k]), r.numpy()), k


@pytest.fixture(scope="module")
def host():
    return host_twin.load("ingest")


def test_half_conversions_of_the_kernel_header_are_exact(host):
    allh = np.arange(65536, dtype=np.uint16)
    out = np.empty(65536, np.float64)
    host.ingest_host_half_to_double(allh.ctypes.data, 65536, out.ctypes.data)
    ref = allh.view(np.float16).astype(np.float64)
    assert np.array_equal(out.view(np.uint64)[~np.isnan(ref)], ref.view(np.uint64)[~np.isnan(ref)]) and np.isnan(out[np.isnan(ref)]).all()
    r = np.random.default_rng(0)
    # doubles around every half value, exact ties between neighbours, subnormals, overflow
    fin = ref[np.isfinite(ref)]
    mids = (fin[:-1] + fin[1:]) / 2
    x = np.concatenate([fin, mids, np.nextafter(mids, np.inf), np.nextafter(mids, -np.inf), r.standard_normal(20000) * 10.0 ** r.integers(-9, 6, 20000),
                        np.array([0.0, -0.0, 65504.0, 65519.99, 65520.0, 1e9, -1e9, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -24, np.inf, -np.inf])])
    got = np.empty(x.size, np.uint16)
    host.ingest_host_double_to_half(np.ascontiguousarray(x).ctypes.data, x.size, got.ctypes.data)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dt", [np.float16, np.float32])
def test_kernel_header_bilinear_equals_numpy_bit_for_bit(host, dt):
    r = np.random.default_rng(3)
    FR, FC, H, N = 112, 16, 256, 4096
    feat = r.standard_normal((FR, FR, FC)).astype(dt)
    xy = np.stack([r.integers(0, H, N), r.integers(0, H, N)], -1).astype(np.int32)
    xy[:4] = [[0, 0], [H - 1, H - 1], [H - 1, 0], [0, H - 1]]
    want = IO.bilinear_interp(feat, xy / H * FR).astype(np.float32)
    got = np.empty((N, FC), np.float32)
    host.ingest_host_bilinear(feat.ctypes.data, int(dt == np.float16), FR, FC, xy.ctypes.data, N, H, got.ctypes.data)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_kernel_header_against_the_reference_fixture(host, gold):
    g, video = gold
    m = g["meta"]
    for case in g["read_raw"]:
        feat = np.ascontiguousarray(video["feature"][case["im0idx"]])
        xy = np.ascontiguousarray(case["xy"].numpy().astype(np.int32))
        got = np.empty((xy.shape[0], feat.shape[-1]), np.float32)
        host.ingest_host_bilinear(feat.ctypes.data, 1, feat.shape[0], feat.shape[-1], xy.ctypes.data, xy.shape[0], m["H"], got.ctypes.data)
        assert np.array_equal(got.view(np.uint32), case["out"]["feature"].numpy().view(np.uint32))
