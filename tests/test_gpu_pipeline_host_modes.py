"""GPU test of the host-buffer `work` entry of the fused handles on its chunked path, in the modes whose chains keep private
per-item records (smoothed items, subspace records, Capon status words, full records): each chunk must read and write them
at ITS item offset, or the two copy/compute lanes overwrite each other's.  work() on host arrays (three chunks over both
lanes) against work_dev() of a second handle in the same mode on the same samples as one batch: every output, every item,
bit for bit."""
import numpy as np
import pytest

import doa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K, M, P, D = 4, 1024, 1, 64, 0.5
N_ITEMS = 2 * ((32 << 20) // (K * N * 8)) + 37          # two full chunks of 1024 items and a third of 37: ~68 MB of samples


@pytest.fixture(scope="module")
def samples():
    x = doa.sim.make_streams(N, N_ITEMS * K, [64.0], D, snr_db=20.0, seed=29)
    x.setflags(write=False)
    return x, [torch.from_numpy(x[k].copy()).cuda() for k in range(N)]


def _music(mode):
    pipe = doa.music_pipeline(N, K, 0, 0, D, M, P, max_batch=N_ITEMS)
    if mode == "capon":
        pipe.set_estimator("capon", 0.0)
    else:
        line = np.stack([D * np.arange(N), np.zeros(N)], axis=1)        # a 4-element line, half a wavelength apart
        pipe.set_steering_table(doa.planar_steering_table(line, P, 0.0, 180.0), 0.0, 180.0)
    return pipe


def _root(mode):
    pipe = doa.root_pipeline(N, K, 0, 0, D, M, max_batch=N_ITEMS)
    if mode == "smoothing":
        pipe.set_spatial_smoothing(3, True)
    else:
        pipe.set_estimator("esprit")
    return pipe


def _bits(a):
    """uint32 view of a float32 / complex64 array: NaN rows compare too"""
    return np.ascontiguousarray(a).view(np.uint32)


# (different fills on the two sides: an output that neither entry wrote does not compare equal)
def _host_out(shape, dtype):
    return np.full(shape, -7.0, dtype)


def _dev_out(shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda")


@pytest.mark.parametrize("handle,mode", [("root", "smoothing"), ("root", "esprit"), ("music", "capon"), ("music", "table")])
def test_chunked_host_entry_equals_one_device_batch(samples, handle, mode):
    x, dev = samples
    n = N_ITEMS
    ptrs = [t.data_ptr() for t in dev]
    st = torch.cuda.current_stream()
    cov_d = _dev_out((n, N * N), torch.complex64)
    on_host, on_dev = (_music(mode), _music(mode)) if handle == "music" else (_root(mode), _root(mode))
    if handle == "music":
        host = [_host_out((n, M), np.float32), _host_out((n, M), np.float32), _host_out((n, N * N), np.complex64),
                _host_out((n, P), np.float32)]
        assert on_host.work(n, [x[k] for k in range(N)], host[0], host[1], cov_out=host[2], spectrum_out=host[3]) == n
        mx_d, am_d, spec_d = _dev_out((n, M), torch.float32), _dev_out((n, M), torch.float32), _dev_out((n, P), torch.float32)
        assert on_dev.work_dev(n, ptrs, cov_d.data_ptr(), spec_d.data_ptr(), mx_d.data_ptr(), am_d.data_ptr(), st) == n
        want = [mx_d, am_d, cov_d, spec_d]
    else:
        host = [_host_out((n, M), np.float32), _host_out((n, N * N), np.complex64)]
        assert on_host.work(n, [x[k] for k in range(N)], host[0], cov_out=host[1]) == n
        ang_d, status_d = _dev_out((n, M), torch.float32), _dev_out((n,), torch.int32)
        assert on_dev.work_dev(n, ptrs, cov_d.data_ptr(), ang_d.data_ptr(), status_d.data_ptr(), st) == n
        want = [ang_d, cov_d]
    torch.cuda.synchronize()
    for got, dev_out in zip(host, want):
        assert np.array_equal(_bits(got), _bits(dev_out.cpu().numpy()))
    if handle == "root":
        assert not status_d.cpu().numpy().any()             # (work() returned n: no item was flagged there either)
