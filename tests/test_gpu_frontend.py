"""The raw-frame front end (csrc/rows.hpp, csrc/warp.hip) against the host model of tests/frontend_model.py on the tables of
tests/frontend_cases.py: the two filters, compact_frames_scan_kernel, sweep_filter_compact_kernel<KITTI> / <!KITTI> and the
three ingest kernels, the last three groups through their C entries.  Every comparison is bit for bit on int32 words; the
one exception is stated in frontend_model: a NaN the KITTI arithmetic PRODUCES is compared as a NaN (its payload is the
implementation's), every copied NaN keeps its payload.  tests/test_frontend_cases_cpu.py proves on the CPU that these tables
reach every class of the kernels' arithmetic and catch every planted fault of the model."""
import numpy as np
import pytest
import torch

import frontend_cases as FC
import frontend_model as FM
import gather_cases as GC
from pwclonet_pylidarslam_amd import _lib, preprocess

pytestmark = pytest.mark.gpu
GUARD = 4                                    # sentinel rows behind every output


def _dev(words, cuda, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(words))
    return (t.view(dtype) if dtype != t.dtype else t).to(cuda)


def _words(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("case", FC.filter_cases(), ids=lambda c: "%s-%s-%s" % (c[0], c[1], "x".join(map(str, c[2]))))
def test_filters_bit_for_bit(cuda, case):
    dataset, calib, shape = case
    pts = FC.filter_input(case)
    assert pts.shape == shape + (4,)
    want_w, want_k = FC.filter_model(case, pts)
    dev = torch.from_numpy(pts).to(cuda)
    if dataset == "kitti":
        xyz, keep = preprocess.transform_filter(dev, FC.CALIBRATIONS[calib])
        got_w, want_w = FM.canon_nan(_words(xyz)), FM.canon_nan(want_w)
    else:
        xyz, keep = preprocess.kitti360_filter(dev, FC.NEAR, FC.GROUND_Z)
        got_w = _words(xyz)
    assert xyz.shape == shape + (3,) and keep.shape == shape and keep.dtype == torch.int32
    got_k = keep.cpu().numpy().reshape(-1)
    assert set(np.unique(got_k)) <= {0, 1}
    bad = np.nonzero(got_k != want_k.astype(np.int32))[0]
    assert len(bad) == 0, (bad[:5], pts.reshape(-1, 4)[bad[:5]])
    bad = np.nonzero((got_w.reshape(-1, 3) != want_w).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], pts.reshape(-1, 4)[bad[:5]])
    assert 0 < want_k.sum() < want_k.size or want_k.size == 1


@pytest.mark.parametrize("n", FC.COMPACT_N)
def test_compact_frames_scan_bit_for_bit(cuda, n):
    """Every b, fill, pattern and cap of the table at n rows; the output buffer is ALL sentinel before the launch (the kernel
    fills nothing: rows past count and the guard rows must still hold it)."""
    lib = _lib.load()
    launches = 0
    for b in FC.COMPACT_B:
        for fill in GC.FILLS:
            xyz = FC.xyz_fill(fill, b, n, n)
            xyz_d = _dev(xyz, cuda)
            for pattern in FC.PATTERNS:
                keep = FC.compact_keep(pattern, b, n)
                keep_d = torch.from_numpy(keep).to(cuda)
                counts_all = [int((keep[f] != 0).sum()) for f in range(b)]
                for cap in FC.caps_for(counts_all, n):
                    buf = np.stack([FC.guard_buffer(cap, 0)] * b)
                    out = torch.from_numpy(np.concatenate((buf.reshape(-1, 3), FC.guard_buffer(0, GUARD)))).to(cuda)
                    counts = torch.full((b + 1,), -7, dtype=torch.int32, device=cuda)
                    _lib.call("compact_frames_scan_kernel_wrapper", cuda, b, n, cap, keep_d.data_ptr(), xyz_d.data_ptr(),
                              out.data_ptr(), counts.data_ptr())
                    launches += 1
                    got, got_c = out.cpu().numpy(), counts.cpu().numpy()
                    where = (n, b, fill, pattern, cap)
                    assert (got[b * cap:] == FC.SENTINEL).all() and got_c[b] == -7, where
                    for f in range(b):
                        want, count = FM.compact_buffer(xyz[f], keep[f], cap, FC.guard_buffer(cap, 1), False)
                        assert got_c[f] == count == min(counts_all[f], cap), where + (f,)
                        assert np.array_equal(got[f * cap:(f + 1) * cap], want[:cap]), where + (f,)
    assert lib.pwclo_last_error() == 0 and launches >= 2 * 2 * 7 * 2


def _sweep_launch(cuda, dataset, batch_d, lengths, cap, packed, counts, trs_d):
    lengths_d = torch.tensor(lengths, dtype=torch.int32, device=cuda)
    _lib.call("sweep_filter_compact_kernel_wrapper", cuda, FC.SWEEP_S, FC.SWEEP_R, cap, lengths_d.data_ptr(), batch_d.data_ptr(),
              0 if dataset == "kitti" else 1, trs_d.data_ptr() if dataset == "kitti" else 0, float(FC.GROUND_Z), float(FC.NEAR),
              packed.data_ptr(), counts.data_ptr())


def _sweep_check(dataset, got, got_c, want, want_c, cap, where):
    canon = FM.canon_nan if dataset == "kitti" else (lambda w: w)
    assert (got[FC.SWEEP_S * cap:] == FC.SENTINEL).all() and got_c[FC.SWEEP_S] == -7, where
    for s in range(FC.SWEEP_S):
        assert got_c[s] == want_c[s], where + (s, got_c[s], want_c[s])
        assert np.array_equal(canon(got[s * cap:(s + 1) * cap]), canon(want[s][:cap])), where + (s,)
        assert not got[s * cap + want_c[s]:(s + 1) * cap].any(), where + (s,)


@pytest.mark.parametrize("dataset", FC.DATASETS)
def test_sweep_filter_compact_is_the_model(cuda, dataset):
    """Four streams per launch with a calibration each; packed prefilled with 7.0 and counts with -1; rows past every length
    hold NaN, or live rows that a kernel reading on would keep; caps around every stream's count.  The reference is the host
    model, not the project's other kernels."""
    trs_d = torch.from_numpy(FC.sweep_trs()).to(cuda)
    launches = 0
    for li, lengths in enumerate(FC.SWEEP_LENGTHS):
        for tail in FC.TAILS:
            batch = FC.sweep_batch(dataset, lengths, tail, 50 + li)
            batch_d = torch.from_numpy(batch).to(cuda)
            for cap in FC.caps_for(FC.sweep_counts(dataset, batch, lengths), FC.SWEEP_R):
                pre = np.concatenate((FC.guard_buffer(FC.SWEEP_S * cap, 0, FC.SWEEP_PREFILL), FC.guard_buffer(0, GUARD)))
                packed = torch.from_numpy(pre).to(cuda)
                counts = torch.tensor([-1] * FC.SWEEP_S + [-7], dtype=torch.int32, device=cuda)
                _sweep_launch(cuda, dataset, batch_d, lengths, cap, packed, counts, trs_d)
                launches += 1
                bufs = [FC.guard_buffer(cap, 1, FC.SWEEP_PREFILL) for _ in lengths]
                want, want_c = FC.sweep_model(dataset, batch, lengths, cap, bufs)
                _sweep_check(dataset, packed.cpu().numpy(), counts.cpu().numpy(), want, want_c, cap, (lengths, tail, cap))
    # a long sweep, then a short one into the same buffer: zero rows past the new counts, no survivor of the long one left
    cap = FC.SWEEP_R
    packed = torch.from_numpy(np.concatenate((FC.guard_buffer(FC.SWEEP_S * cap, 0, FC.SWEEP_PREFILL),
                                              FC.guard_buffer(0, GUARD)))).to(cuda)
    counts = torch.tensor([-1] * FC.SWEEP_S + [-7], dtype=torch.int32, device=cuda)
    bufs = [FC.guard_buffer(cap, 1, FC.SWEEP_PREFILL) for _ in range(FC.SWEEP_S)]
    for k, lengths in enumerate(FC.LONG_THEN_SHORT):
        batch = FC.sweep_batch(dataset, lengths, "nan", 90 + k)
        _sweep_launch(cuda, dataset, torch.from_numpy(batch).to(cuda), lengths, cap, packed, counts, trs_d)
        bufs, want_c = FC.sweep_model(dataset, batch, lengths, cap, bufs)
        _sweep_check(dataset, packed.cpu().numpy(), counts.cpu().numpy(), bufs, want_c, cap, ("long_then_short", k))
    assert max(want_c) < 700 and _lib.load().pwclo_last_error() == 0 and launches >= 2 * len(FC.SWEEP_LENGTHS) * 4


def _ingest_out(rows, cuda):
    return torch.from_numpy(FC.guard_buffer(rows, GUARD)).to(cuda)


@pytest.mark.parametrize("n", FC.INGEST_N)
def test_ingest_kernels_bit_for_bit(cuda, n):
    for fill in GC.FILLS:
        for b in FC.INGEST_B:
            f1, f2 = GC.fill(fill, b, 3, n, 11 * n + b), GC.fill(fill, b, 3, n, 13 * n + b)
            if fill == "identity":
                f2 = (f2.view(np.float32) + np.float32(b * 3 * n)).view(np.int32)     # frame 2 is not frame 1
            out = _ingest_out(2 * b * n, cuda)
            d1, d2 = _dev(f1, cuda), _dev(f2, cuda)                # named: the inputs live until the results are read
            _lib.call("ingest_pairs_kernel_wrapper", cuda, b, n, d1.data_ptr(), d2.data_ptr(), out.data_ptr())
            got = out.cpu().numpy()
            assert np.array_equal(got[:2 * b * n].reshape(2 * b, n, 3), FM.ingest_pairs(f1, f2)), ("pairs", fill, b)
            assert (got[2 * b * n:] == FC.SENTINEL).all()
            for c in FC.INGEST_C:
                for extra in FC.INGEST_EXTRA:
                    nt = n + extra
                    g1, g2 = GC.fill(fill, b, nt, c, 17 * n + c), GC.fill(fill, b, nt, c, 19 * n + c)
                    if fill == "identity":
                        g2 = (g2.view(np.float32) + np.float32(b * nt * c)).view(np.int32)
                    out = _ingest_out(2 * b * n, cuda)
                    d1, d2 = _dev(g1, cuda), _dev(g2, cuda)
                    _lib.call("ingest_frames_kernel_wrapper", cuda, b, n, nt, c, d1.data_ptr(), d2.data_ptr(), out.data_ptr())
                    got = out.cpu().numpy()
                    assert np.array_equal(got[:2 * b * n].reshape(2 * b, n, 3), FM.ingest_frames(g1, g2, n)), ("frames", fill, b, c, nt)
                    assert (got[2 * b * n:] == FC.SENTINEL).all()
        for t in FC.INGEST_T:
            for c in FC.INGEST_C:
                for extra in FC.INGEST_EXTRA:
                    nt = n + extra
                    frames = GC.fill(fill, t, nt, c, 23 * n + c)
                    out = _ingest_out(t * n, cuda)
                    d1 = _dev(frames, cuda)
                    _lib.call("ingest_sequence_kernel_wrapper", cuda, t, n, nt, c, d1.data_ptr(), out.data_ptr())
                    got = out.cpu().numpy()
                    assert np.array_equal(got[:t * n].reshape(t, n, 3), FM.ingest_sequence(frames, n)), ("sequence", fill, t, c, nt)
                    assert (got[t * n:] == FC.SENTINEL).all()
    assert _lib.load().pwclo_last_error() == 0


def test_ingest_refuses_bad_shapes_and_writes_nothing(cuda):
    """c = 2 and n_total < n: the library's error, the output untouched."""
    n, b = 257, 2
    src = _dev(GC.fill("identity", b, n, 5, 1), cuda)
    for entry, head in (("ingest_frames_kernel_wrapper", (b,)), ("ingest_sequence_kernel_wrapper", (b,))):
        two = entry == "ingest_frames_kernel_wrapper"
        for n_total, c in ((n, 2), (n - 1, 3)):
            out = _ingest_out(2 * b * n, cuda)
            args = head + (n, n_total, c, src.data_ptr()) + ((src.data_ptr(),) if two else ()) + (out.data_ptr(),)
            with pytest.raises(RuntimeError, match="need c >= 3 and n_total >= n"):
                _lib.call(entry, cuda, *args)
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == FC.SENTINEL).all(), (entry, n_total, c)
    assert _lib.load().pwclo_last_error() == 0
