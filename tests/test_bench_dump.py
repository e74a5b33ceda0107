"""bench.py --dump-outputs DIR: what the last timed step handed its caller, as DIR/<name>.npy in float64, under 64 MB in
all, the same on every run with the same arguments -- so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    coef = np.linspace(-1, 1, 1000, dtype=np.float32)
    out = dict(p=np.array([0.25]), coef=coef, coef_fdr=np.arange(1000.0))
    written = bench.dump_outputs(str(tmp_path / 'd'), out)
    assert written == dict(p=[1, 1], coef=[1000, 1000], coef_fdr=[1000, 1000])
    assert sorted(os.listdir(tmp_path / 'd')) == ['coef.npy', 'coef_fdr.npy', 'p.npy']
    for name, a in out.items():
        got = np.load(tmp_path / 'd' / (name + '.npy'))
        assert got.dtype == np.float64
        assert np.array_equal(got, a.astype(np.float64))


def test_large_outputs_are_a_fixed_sample_under_the_limit(tmp_path):
    limit = 1 << 20
    big = np.arange(400_000, dtype=np.float64)                 # 3.2 MB each: both sampled
    out = dict(p=np.array([0.5]), coef=big, coef_fdr=-big)
    w1 = bench.dump_outputs(str(tmp_path / 'a'), out, limit=limit)
    w2 = bench.dump_outputs(str(tmp_path / 'b'), out, limit=limit)
    assert w1 == w2 and w1['p'] == [1, 1] and 0 < w1['coef'][0] < 400_000 and w1['coef'][1] == 400_000
    assert _sizes(tmp_path / 'a') <= limit
    for name in out:
        a, b = np.load(tmp_path / 'a' / (name + '.npy')), np.load(tmp_path / 'b' / (name + '.npy'))
        assert np.array_equal(a, b)                            # the same positions on every run
    sample = np.load(tmp_path / 'a' / 'coef.npy')
    assert np.all(np.diff(sample) > 0)                         # ascending positions, no repeats
    assert np.array_equal(np.load(tmp_path / 'a' / 'coef_fdr.npy'), -sample)


def test_the_default_workload_is_dumped_whole():
    n = bench.WORKLOADS['C4'][0]
    assert n <= bench.DUMP_LIMIT_BYTES // 3 // 8 - 512 and bench.DUMP_LIMIT_BYTES < 64_000_000


def _bench(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--workload', 'C2', '--steps', '2',
                        '--warmup', '1', '--no-extra', '--no-cpu-baseline', '--details', os.path.join(out_dir, 'details.json'),
                        '--dump-outputs', os.path.join(out_dir, 'dump')],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, 'dump', f)) for f in os.listdir(os.path.join(out_dir, 'dump'))}


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_on_every_run(tmp_path):
    os.makedirs(tmp_path / 'a')
    os.makedirs(tmp_path / 'b')
    line, a = _bench(str(tmp_path / 'a'))
    _, b = _bench(str(tmp_path / 'b'))
    n = bench.WORKLOADS['C2'][0]
    assert sorted(a) == ['coef', 'coef_fdr', 'p']
    assert a['p'].shape == (1,) and a['coef'].shape == (n,) and a['coef_fdr'].shape == (n,)
    assert all(v.dtype == np.float64 for v in a.values())
    assert a['p'][0] == line['config']['p_value']
    assert line['steps'] == 2 and line['ms_per_step'] > 0
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
