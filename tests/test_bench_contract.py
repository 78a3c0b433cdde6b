"""bench.py end to end on the numpy emulation of the device (tiny chain): the JSON line must keep the driver's contract
(keys, types, the `roofline` and `cpu_baseline` objects) and the engine wiring bench.py relies on must not rot.  The
numbers mean nothing here -- the kernels are emulated; on the MI355X the same code path produces the round's bench line."""
import contextlib
import io
import json
import sys

import pytest


def test_bench_json_contract(monkeypatch):
    import mock_device
    mock_device.install(monkeypatch)
    import torch
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--L', '12', '--chi', '16', '--steps', '2', '--warmup', '1', '--cpu-sample-bonds', '1', '--full'])
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    import bench
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    lines = [l for l in buf.getvalue().splitlines() if l.strip()]
    # the contract line is the LAST line and short; everything long precedes it, tagged (round 4's single 27 KB line was cut off
    # by the driver's capture: BENCH_r04.json "parsed": null)
    assert all(json.loads(l).get('bench_detail') for l in lines[:-1])
    assert len(lines[-1]) < 4096
    out = json.loads(lines[-1])
    assert 'bench_detail' not in out
    detail = json.loads(lines[0])
    assert detail['bench_detail'] == 'headline' and 'svd' in detail['roofline']['kernel'] and detail['value'] == pytest.approx(out['value'], rel=1e-5)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in out, k
    assert out['n_gpus'] == 1 and out['steps'] == 2 and out['warmup'] == 1
    assert out['higher_is_better'] is False and out['vs_baseline'] is None and out['dtype'] == 'f64'
    assert out['unit'] == 's/sweep' and out['value'] > 0 and abs(out['ms_per_step'] - 1e3 * out['value']) < 1e-3 * out['ms_per_step']
    assert 'workload' in out['config'] and 'model' not in out['config']
    r = out['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r, k
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] in ('GB/s', 'TFLOP/s') and r['peak'] > 0
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-4 * r['frac']
    c = out['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in c, k
    assert c['kind'] in ('reference', 'port') and c['value'] > 0
    # parity at scale rides on the same line ("report parity at scale in the bench line")
    assert out['matvec_max_rel_err'] < 1e-10 and out['sv_max_rel_err'] < 1e-10 and out['E0_rel_err'] < 1e-10
    assert 'energy_err' in out and 'roofline_gemm' in out
    assert 'svd' in r['kernel'] and r['launches'] > 0
    assert abs(out['E'] - (-5.142090632841)) < 1e-6          # XXZ Jz=1, L=12 ground state energy (exact: -5.1420906328)
    assert out['sv_kept'] > 0 and out['sv_kept_rel_err_over_1e-10'] == 0


def _bench_in_process(monkeypatch, argv):
    import mock_device
    mock_device.install(monkeypatch)
    import torch
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: None)
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    import bench
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    return json.loads([l for l in buf.getvalue().splitlines() if l.strip()][-1])


@pytest.mark.parametrize("config", ["heis2048", "tebd1024"])
def test_bench_plain_run_is_lean(monkeypatch, config):
    """Without --full the run is set-up, warm-up, the timed steps and the line: no CPU baseline, no parity sample, no extra leg --
    and the headline fields still mean what they do with --full."""
    import bench

    def must_not_run(*a, **k):
        raise AssertionError("a plain run must not do this")
    for name in ('parity_and_port', 'reference_same_run', 'extras', 'vector_roofline'):
        monkeypatch.setattr(bench, name, must_not_run)
    out = _bench_in_process(monkeypatch, ['--config', config, '--L', '12', '--chi', '16', '--steps', '3', '--warmup', '1'])
    assert out['steps'] == 3 and out['warmup'] == 1 and out['n_gpus'] == 1 and out['higher_is_better'] is False
    assert out['value'] > 0 and abs(out['ms_per_step'] - 1e3 * out['value']) < 1e-3 * out['ms_per_step']
    assert 'cpu_baseline' not in out and 'sv_max_rel_err' not in out and 'other_configs' not in out and 'tebd_parity' not in out
    assert 'roofline' in out and 'roofline_gemm' in out
    if config == 'heis2048':
        assert out['unit'] == 's/sweep' and out['dtype'] == 'f64' and 'energy_err' in out
        assert abs(out['E'] - (-5.142090632841)) < 1e-6
    else:
        assert out['unit'] == 's/step' and out['dtype'] == 'c128' and out['S_mid_entropy'] > 0


def test_bench_steps_sets_the_timed_steps(monkeypatch):
    """--steps K runs exactly K timed sweeps after the ramp and the W warm-up sweeps."""
    import bench
    sweeps = []
    real = bench.build_dmrg

    def counting(*a, **k):
        eng, E = real(*a, **k)
        sweep = eng.sweep
        eng.sweep = lambda: sweeps.append(1) or sweep()
        sweeps.clear()
        return eng, E
    monkeypatch.setattr(bench, 'build_dmrg', counting)
    out = _bench_in_process(monkeypatch, ['--L', '12', '--chi', '16', '--steps', '4', '--warmup', '2'])
    assert out['steps'] == 4 and len(sweeps) == 4 + 2


def test_bench_dump_outputs(monkeypatch, tmp_path):
    """--dump-outputs DIR: float64 .npy files of what the last timed step computed, the same in two runs with the same arguments
    (fixed inputs), and consistent with the line."""
    import numpy as np
    runs = []
    for k in range(2):
        d = tmp_path / ('run%d' % k)
        out = _bench_in_process(monkeypatch, ['--L', '12', '--chi', '16', '--steps', '2', '--warmup', '1', '--dump-outputs', str(d)])
        runs.append({p.stem: np.load(p) for p in sorted(d.glob('*.npy'))})
    a, b = runs
    assert set(a) == {'energy', 'bond_energies', 'bond_trunc_err', 'schmidt_values', 'mps_tensors_sample'}
    assert sum(v.nbytes for v in a.values()) < 64 << 20
    for name in a:
        assert a[name].dtype == np.float64 and a[name].size > 0, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert a['energy'][0] == out['E'] and a['bond_energies'].shape == (2 * (12 - 2),) and a['bond_energies'][-1] == out['E']
    S = a['schmidt_values']
    assert S.shape[0] == 13 and S.shape[1] <= 16
    np.testing.assert_allclose(np.sum(S[1:-1] ** 2, axis=1), 1., rtol=1e-10)
    assert np.all(np.isfinite(a['mps_tensors_sample'])) and np.any(a['mps_tensors_sample'] != 0)


def test_bench_dump_outputs_tebd(monkeypatch, tmp_path):
    """The TEBD configuration (complex128 tensors) dumps float64 too: complex entries as (real, imag) pairs."""
    import numpy as np
    out = _bench_in_process(monkeypatch, ['--config', 'tebd1024', '--L', '12', '--chi', '16', '--steps', '1', '--warmup', '1',
                                          '--dump-outputs', str(tmp_path)])
    got = {p.stem: np.load(p) for p in tmp_path.glob('*.npy')}
    assert set(got) == {'schmidt_values', 'mps_tensors_sample', 'trunc_err', 'norm'}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got['trunc_err'][0] == pytest.approx(out['trunc_err_eps'], rel=1e-5) and got['mps_tensors_sample'].size % 2 == 0


def test_compact_line_fits_with_all_extras():
    """Round 4's full line (profiles/r04_bench_heis2048.json: headline + every extra leg, 27 KB) through `bench.compact`: the contract
    line stays under 4 KB and still carries the contract keys, both rooflines, the CPU baseline, the parity fields and one number
    per extra leg."""
    import os
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'profiles', 'r04_bench_heis2048.json')) as f:
        full = json.load(f)
    assert len(json.dumps(full)) > 20000
    c, line = bench.compact(full)
    assert len(line) < 4096 and json.loads(line) == c
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'roofline_gemm', 'cpu_baseline', 'energy_err', 'sv_max_rel_err', 'matvec_max_rel_err',
              'E0_rel_err', 'other_configs', 'module_form', 'lanczos_adaptive'):
        assert k in c, k
    assert c['E'] == full['E']                                      # energies are not rounded
    assert abs(c['roofline']['frac'] - full['roofline']['frac']) < 1e-5 * full['roofline']['frac']
    assert set(c['other_configs']) == set(full['other_configs']) and c['other_configs']['xxz512']['value'] > 0
    assert c['lanczos_adaptive']['s_per_sweep'] > 0 and len(c['roofline']['kernel']) <= 120
    # the guard of last resort: optional parts go before the line grows
    full['config']['workload'] = full['config']['workload'] * 20
    full['other_configs'] = {('cfg%d' % i): dict(v) for i, v in enumerate(list(full['other_configs'].values()) * 20)}
    c2, line2 = bench.compact(full)
    assert len(line2) < 4096 and 'roofline' in c2 and 'value' in c2


def test_bench_gpus_flag_launches_ranks(tmp_path):
    """`python bench.py --gpus 2` as the driver may run it: NO rendezvous variables in the environment -- bench.py launches its own two
    ranks (torch.distributed.run on 127.0.0.1) and rank 0 prints the contract line with n_gpus == 2.  gloo + the emulated device
    (tests/mock_site/sitecustomize.py); on the MI355X node the same code path runs RCCL."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(PYTHONPATH=os.path.join(root, 'tests', 'mock_site') + os.pathsep + env.get('PYTHONPATH', ''), TPA_TEST_MOCK_DEVICE='1',
               TPA_BENCH_BACKEND='gloo', OMP_NUM_THREADS='1')
    pr = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--L', '12', '--chi', '16', '--steps', '1', '--warmup', '1'],
                        env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith('{')]
    out = json.loads(lines[-1])
    assert 'bench_detail' not in out and out['n_gpus'] == 2 and out['scaling'] == 'strong' and out['value'] > 0
    assert 'Amdahl' in out['config']['parallelism']
    assert out['lanczos_stats']['n_native_sharded'] > 0             # the one-call Lanczos with the collective as a program op, on both ranks
    assert abs(out['E'] - (-5.142090632841)) < 1e-6


def _bench_worker(rank, world, port, ret):
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      TPA_BENCH_BACKEND='gloo')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tests'))
    try:
        from _pytest.monkeypatch import MonkeyPatch
        import mock_device
        mp = MonkeyPatch()
        mock_device.install(mp)
        import torch
        mp.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
        mp.setattr(torch.cuda, 'set_device', lambda *a, **k: None)
        sys.argv = ['bench.py', '--gpus', str(world), '--L', '12', '--chi', '16', '--steps', '1', '--warmup', '1'] + os.environ.get('TPA_TEST_BENCH_ARGS', '').split()
        import bench
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            bench.main()
        ret[rank] = buf.getvalue()
    except Exception:  # pragma: no cover
        import traceback
        ret[rank] = 'FAIL: ' + traceback.format_exc()


def test_bench_two_ranks_gloo():
    """The N>1 control flow of bench.py (rendezvous, sharded engine, barriers, max over ranks, rank 0 prints ONE line)
    with world_size 2 over gloo on the emulated device."""
    import os
    import torch.multiprocessing as tmp
    world = 2
    port = 29700 + (os.getpid() % 200)
    mgr = tmp.Manager()
    ret = mgr.dict()
    tmp.spawn(_bench_worker, args=(world, port, ret), nprocs=world, join=True)
    assert not any(str(ret.get(r, 'FAIL')).startswith('FAIL') for r in range(world)), dict(ret)
    lines = [l for l in ret[0].splitlines() if l.strip()]
    assert len(lines) >= 1 and ret[1].strip() == ''
    out = json.loads(lines[-1])
    assert out['n_gpus'] == 2 and out['scaling'] == 'strong' and 'cpu_baseline' not in out
    assert 'sharded' in out['config']['parallelism'] and out['value'] > 0
    assert abs(out['E'] - (-5.142090632841)) < 1e-6


def test_bench_two_ranks_gloo_tebd(monkeypatch):
    """``bench.py --config tebd1024 --gpus 2`` (tiny chain, emulated device): the bond-sharded TEBD engine under the bench's N > 1
    control flow; the line reports the state every rank holds."""
    import os
    import torch.multiprocessing as tmp
    monkeypatch.setenv('TPA_TEST_BENCH_ARGS', '--config tebd1024 --no-cpu-baseline')
    world = 2
    port = 29300 + (os.getpid() % 200)
    mgr = tmp.Manager()
    ret = mgr.dict()
    tmp.spawn(_bench_worker, args=(world, port, ret), nprocs=world, join=True)
    assert not any(str(ret.get(r, 'FAIL')).startswith('FAIL') for r in range(world)), dict(ret)
    out = json.loads([l for l in ret[0].splitlines() if l.strip()][-1])
    assert out['n_gpus'] == 2 and out['unit'] == 's/step' and 'dealt over 2 GPUs' in out['config']['parallelism']
    assert out['S_mid_entropy'] > 0 and out['value'] > 0


def test_smoke_runs_on_the_emulated_device(monkeypatch, capsys):
    """__graft_entry__.smoke() (DMRG energy vs the exact value, matvec and SVD vs the oracle) with the device entry points
    emulated: guards the wiring the driver runs on the MI355X at round end."""
    import mock_device
    mock_device.install(monkeypatch)
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: None)
    import __graft_entry__ as g
    g.smoke()
    assert 'smoke ok' in capsys.readouterr().out


def test_bench_force_dist_one_rank(tmp_path):
    """`bench.py --force-dist` (what tests/test_sharded.py::test_rccl_collective_world1 runs over RCCL on the MI355X), here over gloo on
    the emulated device: a process group of ONE rank, the row-sharded operator forced, the all-gather issued from the collective
    callback of the native Lanczos run -- and the same energy as the plain run."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'TPA_SHARD_FORCE')}
    env.update(PYTHONPATH=os.path.join(root, 'tests', 'mock_site') + os.pathsep + env.get('PYTHONPATH', ''), TPA_TEST_MOCK_DEVICE='1',
               TPA_BENCH_BACKEND='gloo', OMP_NUM_THREADS='1')
    outs = []
    for extra in (['--force-dist'], []):
        pr = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--L', '12', '--chi', '16', '--steps', '1', '--warmup', '1',
                             '--no-cpu-baseline', '--no-extras'] + extra, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert pr.returncode == 0, pr.stderr[-3000:]
        outs.append(json.loads([l for l in pr.stdout.splitlines() if l.startswith('{')][-1]))
    forced, plain = outs
    assert forced['n_gpus'] == 1 and 'ONE rank' in forced['config']['parallelism'] and forced['lanczos_stats']['n_native_sharded'] > 0
    assert plain['lanczos_stats']['n_native_sharded'] == 0
    assert abs(forced['E'] - plain['E']) < 1e-12 * abs(plain['E'])
