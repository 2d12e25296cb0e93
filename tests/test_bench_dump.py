"""bench.py --dump-outputs: the arrays written for an ATZ1 in HBM (bench.dump_outputs) against a host
restatement, for an output handed over as a device pointer (one GPU) and as a tensor (the N > 1 file mode),
below and above the sampling threshold, at lengths that are no multiple of the block size."""
import os

import numpy as np
import pytest

ST = {"file_bytes": 123456789, "n_streams": 77, "n_recomp": 70, "atz_bytes": 0}


def expected(host, n):
    import bench
    a = host[:n]
    if n > bench.DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(0).integers(0, n, size=bench.DUMP_SAMPLE))
        sample = a[idx]
    else:
        sample = a
    pad = (-n) % bench.DUMP_BLOCK
    sums = np.concatenate([a, np.zeros(pad, np.uint8)]).reshape(-1, bench.DUMP_BLOCK).sum(axis=1, dtype=np.int64)
    return sample.astype(np.float32), sums.astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("as_pointer", [True, False])
@pytest.mark.parametrize("n", [1, 65536, 3 * 65536 + 17, 8 * 1000 * 1000 + 12345])
def test_dump_outputs(tmp_path, n, as_pointer):
    import torch
    import bench
    host = np.random.default_rng(n).integers(0, 256, size=n + 100, dtype=np.uint8)   # 100 bytes past the ATZ1's end
    dev = torch.from_numpy(host).to("cuda")
    st = dict(ST, atz_bytes=n)
    bench.dump_outputs(str(tmp_path), dev.data_ptr() if as_pointer else dev, n, st)
    got = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in sorted(os.listdir(str(tmp_path)))}
    assert sorted(got) == ["atz_block_sums", "atz_len", "atz_sample", "counts"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 * 1000 * 1000
    sample, sums = expected(host, n)
    assert got["atz_len"].tolist() == [float(n)]
    assert got["atz_sample"].shape == (min(n, bench.DUMP_SAMPLE),) and np.array_equal(got["atz_sample"], sample)
    assert np.array_equal(got["atz_block_sums"], sums)
    assert got["counts"].tolist() == [123456789.0, 77.0, 70.0, float(n)]
