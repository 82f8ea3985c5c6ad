"""What the GPU tests of signal conditioning share (tests/test_gpu_preprocess.py, tests/test_gpu_preprocess_shapes.py): a
call of hmmbw_preprocess on a ragged batch with guarded buffers and optional base-pointer offsets, a call of
hmmbw_window_overlap, and the comparison of a call's results with the restatement (tests/preprocess_ref.py)."""
import ctypes

import numpy as np

import preprocess_ref as R

MODES = {"batch": (R.BATCH, False, "batch_bounds", "batch_trimmed"), "live": (R.LIVE, True, "live_bounds", "live_windowed")}
PAD = 4          # spare elements on each side of the samples and of filtered_out: a multiple of every vector width
X_FILL, Y_FILL = 77, -7.0


def p(t, shift=0):
    return ctypes.c_void_p(t.data_ptr() + shift * t.element_size())


def offsets_of(signals):
    return np.concatenate([[0], np.cumsum([len(R.column(s)) for s in signals])]).astype(np.int64)


def preprocess(signals, factors, as_f64, host_offsets=True, win=320, hop=160, stats=True, coeff=R.COEFF, x_shift=0,
               y_shift=0):
    """hmmbw_preprocess on the concatenated columns; returns (status, y, bounds, stats, offsets) as host arrays.
    ``x_shift`` / ``y_shift`` move the base of samples / filtered_out by that many elements off the allocator's
    alignment.  Both buffers have PAD spare elements on each side; those of filtered_out must keep their fill."""
    import torch

    from hmm_training_amd import _lib
    assert 0 <= x_shift <= PAD and 0 <= y_shift <= PAD
    cols = [R.column(s) for s in signals]
    offs = offsets_of(signals)
    x = np.concatenate(cols)
    x = x.astype(np.float64) if as_f64 else x.astype(np.int16)
    n = len(x)
    xbuf = np.full(n + 2 * PAD, X_FILL, dtype=x.dtype)
    xbuf[PAD + x_shift:PAD + x_shift + n] = x
    tx, toff = torch.from_numpy(xbuf).cuda(), torch.from_numpy(offs).cuda()
    y = torch.full((n + 2 * PAD,), Y_FILL, dtype=torch.float64, device="cuda")
    bounds = torch.full((len(cols), 2), -7, dtype=torch.int64, device="cuda")
    nf = sum(max(R.frame_count(len(c), win, hop), 0) for c in cols) if 1 <= hop else 0
    st = torch.full((max(nf, 1), 2), -7.0, dtype=torch.float64, device="cuda")
    fac = np.array(factors, dtype=np.float64)
    rc = _lib.lib().hmmbw_preprocess(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(tx, PAD + x_shift),
                                     _lib.SAMPLES_F64 if as_f64 else _lib.SAMPLES_I16, p(toff),
                                     ctypes.c_void_p(offs.ctypes.data) if host_offsets else None, len(cols), coeff,
                                     win, hop, ctypes.c_void_p(fac.ctypes.data), p(y, PAD + y_shift), p(bounds),
                                     p(st) if stats else None)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    a = PAD + y_shift
    assert np.all(yh[:a] == Y_FILL) and np.all(yh[a + n:] == Y_FILL), "filtered_out: a store outside the samples"
    return rc, yh[a:a + n].copy(), bounds.cpu().numpy(), st.cpu().numpy()[:nf], offs


def window_overlap(x, offs, bounds, table, whop):
    """hmmbw_window_overlap in place on a copy of the host array x; returns (status, result)"""
    import torch

    from hmm_training_amd import _lib
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    toff = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)).cuda()
    tw = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).cuda()
    rc = _lib.lib().hmmbw_window_overlap(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(t), p(toff), p(tb),
                                         len(offs) - 1, p(tw), len(table), whop)
    torch.cuda.synchronize()
    return rc, t.cpu().numpy()


def check_against(wants, y, bounds, stats, offs, trimmed=None, rtol=R.POWER_RTOL, names=None):
    """the results of one call against the restatement's dict of every recording (preprocess_ref.preprocess): y, zcr,
    bounds and the trimmed signal for equality, power within rtol.  Returns the largest relative power difference."""
    pos, worst = 0, 0.0
    for r, want in enumerate(wants):
        name = names[r] if names is not None else r
        lo, hi = offs[r], offs[r + 1]
        if y is not None:
            # the whole of the recording, bit for bit: a fused multiply-add fails here, and so does a first sample
            # that saw its neighbour's last one
            assert np.array_equal(y[lo:hi], want["y"]), name
            assert y[lo] == 0.0
        assert bounds[r].tolist() == [want["start"], want["finish"]], name
        nf = len(want["zcr"])
        assert np.array_equal(stats[pos:pos + nf, 0], want["zcr"]), name
        power = stats[pos:pos + nf, 1]
        scale = np.where(want["power"] > 0, want["power"], 1.0)
        rel = float((np.abs(power - want["power"]) / scale).max())
        assert rel <= rtol, (name, rel)
        worst = max(worst, rel)
        pos += nf
        if trimmed is not None:
            assert trimmed[r].shape == (len(want["out"]), 1) and trimmed[r].dtype == np.float64
            assert np.array_equal(trimmed[r][:, 0], want["out"]), name
    assert pos == len(stats)
    return worst
