"""bench.py --dump-outputs on the host: bench.dump_outputs writes float32 / float64 .npy files, caps the set at DUMP_LIMIT_BYTES with the
same fixed, seeded sample of rows from every array, and gives the same files from two calls on the same arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_had_ipc = 'HSA_ENABLE_IPC_MODE_LEGACY' in os.environ
import bench  # noqa: E402
if not _had_ipc:
    os.environ.pop('HSA_ENABLE_IPC_MODE_LEGACY', None)        # (bench.py sets it for its own process; this one keeps its environment)


def _arrays(n):
    rng = np.random.default_rng(7)
    return {'obs': rng.normal(size=(n, 207)).astype(np.float32), 'reward': rng.normal(size=n).astype(np.float32),
            'done': rng.integers(0, 2, size=n).astype(bool), 'why': rng.integers(0, 4, size=n).astype(np.uint8),
            'state': rng.normal(size=(n, 37)).astype(np.float32), 'time': rng.uniform(size=n)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_set_is_written_whole_with_float_dtypes(tmp_path):
    a = _arrays(256)
    bench.dump_outputs(str(tmp_path), a)
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(a)                                         # no sample index when nothing was sampled
    for k, v in a.items():
        want = np.float64 if v.dtype == np.float64 else np.float32
        assert got[k].dtype == want and got[k].shape == v.shape
        np.testing.assert_array_equal(got[k], v.astype(want))               # bool / uint8 -> 0.0 / 1.0 / small integers, floats unchanged


def test_large_set_is_capped_with_the_same_rows_from_every_array(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 1 << 20)
    n = 8192
    a = _arrays(n)
    assert sum(v.nbytes for v in a.values()) > bench.DUMP_LIMIT_BYTES
    d1, d2 = str(tmp_path / 'one'), str(tmp_path / 'two')
    bench.dump_outputs(d1, a)
    bench.dump_outputs(d2, a)
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= bench.DUMP_LIMIT_BYTES
    g1, g2 = _load(d1), _load(d2)
    assert sorted(g1) == sorted(list(a) + ['sampled_rows'])
    rows = g1['sampled_rows'].astype(np.int64)
    assert rows.size > 0 and (np.diff(rows) > 0).all() and rows[-1] < n
    for k, v in a.items():
        want = np.float64 if v.dtype == np.float64 else np.float32
        assert g1[k].dtype == want and g1[k].shape == (rows.size,) + v.shape[1:]
        np.testing.assert_array_equal(g1[k], v[rows].astype(want))         # every array sampled at the same rows
    for k in g1:                                                            # two calls: the same sample, the same bytes
        np.testing.assert_array_equal(g1[k], g2[k])


def test_default_cap_is_64_mb():
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
