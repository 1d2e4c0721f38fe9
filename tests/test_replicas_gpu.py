"""Replicas of the device samplers on real engines (vega_amd/replicas.py): replica r is the plain sampler on Philox stream r,
bit for bit; two rank processes sharing the one GPU write the merged files one process writes; ``replicas = 1`` writes the
files of a config without the key; merged nested replicas give the exact evidence and posterior of parameters the model is
linear in; two ensembles give a finite R-hat and getdist's ``name_1.txt``, ``name_2.txt``."""
import configparser
import socket
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, run_programs

pytestmark = pytest.mark.gpu

SETTINGS = {'Ensemble': {'walkers': '16', 'steps': '20', 'seed': '4'},
            'Nested': {'num_live': '64', 'num_repeats': '4', 'threads': '16', 'seed': '4', 'max_iterations': '5'},
            'SMC': {'particles': '128', 'sweeps': '4', 'seed': '4', 'max_stages': '3'}}
FINAL = ('.txt', '.paramnames', '.stats')


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _config(tmp_path, tag, sampler, replicas=None, **changes):
    """configs/<tag>/main.ini under ``tmp_path``: the auto config with the sampler's section; (config, output folder)."""
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = sampler
    out = tmp_path / f'chains_{tag}'
    out.mkdir()
    cfg[sampler] = dict(SETTINGS[sampler], path=str(out), name='run', **changes)
    if replicas is not None:
        cfg[sampler]['replicas'] = str(replicas)
    (tmp_path / 'configs' / tag).mkdir(parents=True)
    with open(tmp_path / 'configs' / tag / 'main.ini', 'w') as f:
        cfg.write(f)
    return f'configs/{tag}/main.ini', out


def _run(tmp_path, config):
    from vega_amd import run_vega_sampler
    return run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None, rank=0, world_size=1)


def _final_files(folder):
    return {p.name: p.read_bytes() for p in folder.iterdir() if p.suffix in FINAL}


@pytest.mark.parametrize('sampler', ['Ensemble', 'Nested', 'SMC'])
def test_a_replica_is_the_plain_sampler_on_its_stream(tmp_path, sampler):
    from vega_amd import EnsembleSampler, NestedSampler, SMCSampler
    from vega_amd import replicas as rep
    config, folder = _config(tmp_path, 'two', sampler, replicas=2)
    out = _run(tmp_path, config)
    vega = out.samplers[0].vega
    try:
        assert out.replicas == 2 and out.block == (0, 2) and all(s.driver == 'device' for s in out.samplers)
        recs = [rep.load_record(rep.record_path(folder, 'run', r)) for r in range(2)]
        for r, rec in enumerate(recs):
            assert rec['stream'] == r and rec['seed'] == 4 and rec['driver'] == 'device'
            if sampler == 'Nested':
                plain = NestedSampler(vega, num_live=64, num_repeats=4, threads=16, seed=4, max_iterations=5, stream=r).run()
                want = dict(zip(('dead_u', 'dead_lnl', 'dead_nlive'), plain.dead()), live_u=plain.live_u, live_lnl=plain.live_lnl,
                            points=plain.samples()[0])
            elif sampler == 'SMC':
                plain = SMCSampler(vega, particles=128, sweeps=4, seed=4, max_stages=3, stream=r).run()
                want = dict(u=plain.u, lnl=plain.lnl, stage_beta=plain.stages['beta'], points=plain.samples()[0],
                            stage_lnl=np.array([s['lnl'] for s in plain.record]), stage_anc=np.array([s['anc'] for s in plain.record]))
            else:
                plain = EnsembleSampler(vega, 16, seed=4, stream=r).run(20)
                want = dict(chain=plain.get_chain(), chain_lnl=plain.get_log_lik(), accepted=plain.accepted, points=plain.get_chain())
            assert plain.driver == 'device'
            for key, val in want.items():
                assert np.array_equal(rec[key], val), (r, key)
            assert rec['stats']['rows' if sampler != 'Ensemble' else 'proposals'] == plain.stats['rows' if sampler != 'Ensemble' else 'proposals']
        assert not np.array_equal(recs[0]['points'], recs[1]['points'])
        # the device driver on stream 1 is the restatement on stream 1 (the key word reaches the kernels)
        if sampler == 'Nested':
            py = NestedSampler(vega, num_live=64, num_repeats=4, threads=16, seed=4, max_iterations=5, stream=1, driver='python').run()
            assert np.array_equal(py.dead()[0], recs[1]['dead_u']) and np.array_equal(py.live_u, recs[1]['live_u'])
        elif sampler == 'SMC':
            py = SMCSampler(vega, particles=128, sweeps=4, seed=4, max_stages=3, stream=1, driver='python').run()
            assert np.array_equal(py.u, recs[1]['u'])
        else:
            py = EnsembleSampler(vega, 16, seed=4, stream=1, driver='python').run(20)
            assert np.array_equal(py.get_chain(), recs[1]['chain'])
    finally:
        vega.close()


@pytest.mark.parametrize('sampler', ['Nested', 'SMC'])
def test_two_ranks_on_one_gpu_write_what_one_process_writes(tmp_path, sampler):
    config2, folder2 = _config(tmp_path, 'ranks', sampler, replicas=4)
    config1, folder1 = _config(tmp_path, 'alone', sampler, replicas=4)
    port = _free_port()
    argv = [sys.executable, str(REPO / 'scripts' / 'run_vega_sampler.py'), config2, '--search-dir', str(tmp_path), '--search-dir',
            str(GOLDEN)]
    envs = [{'RANK': str(r), 'WORLD_SIZE': '2', 'LOCAL_RANK': str(r), 'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port),
             'HSA_ENABLE_IPC_MODE_LEGACY': '0'} for r in range(2)]
    results = run_programs([argv, argv], envs, timeout=600)
    for rank, (rc, output) in enumerate(results):
        assert rc == 0, f'rank {rank} failed:\n{output[-4000:]}'
    assert '4 replicas on 2 rank(s)' in results[0][1] and '4 replicas' not in results[1][1]
    out = _run(tmp_path, config1)
    out.samplers[0].vega.close()
    assert out.counts[0][0] == 4
    one, two = _final_files(folder1), _final_files(folder2)
    assert set(one) == set(two) == {'run.txt', 'run.paramnames', 'run.stats'}
    for name in one:
        assert one[name] == two[name], name
    assert sorted(p.name for p in folder2.glob('*.npz')) == [f'run.replica{r}.npz' for r in range(4)]


@pytest.mark.parametrize('sampler', ['Ensemble', 'Nested', 'SMC'])
def test_one_replica_is_the_output_of_today(tmp_path, sampler):
    config_a, folder_a = _config(tmp_path, 'absent', sampler)
    config_b, folder_b = _config(tmp_path, 'one', sampler, replicas=1)
    a = _run(tmp_path, config_a)
    a.vega.close()
    b = _run(tmp_path, config_b)
    b.vega.close()
    assert type(a) is type(b) and b.stream == 0
    want = {'run.txt', 'run.paramnames'} | ({'run.stats'} if sampler != 'Ensemble' else set())
    assert {p.name for p in folder_b.iterdir()} == want == {p.name for p in folder_a.iterdir()}
    assert _final_files(folder_a) == _final_files(folder_b)


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _linear_gaussian(auto_vega):
    """F, b*, lnL(b*) of 4 additive broadband coefficients (chi2 is exactly quadratic in them) from second differences (as in
    tests/test_nested_gpu.py)."""
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
    cols = [auto_vega.param_names.index(n) for n in names]
    base = auto_vega._theta(None)
    b0 = base[cols].copy()

    def chi2_at(offsets):
        th = np.repeat(base[None, :], len(offsets), axis=0)
        th[:, cols] = b0 + np.asarray(offsets)
        return auto_vega.chi2_batch(th)

    def fit(delta):
        n = len(cols)
        pts = [np.zeros(n)] + [delta * np.eye(n)[i] for i in range(n)] + [2 * delta * np.eye(n)[i] for i in range(n)]
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        pts += [delta * (np.eye(n)[i] + np.eye(n)[j]) for i, j in pairs]
        c = chi2_at(pts)
        F = np.zeros((n, n))
        for i in range(n):
            F[i, i] = (c[1 + n + i] - 2 * c[1 + i] + c[0]) / (2 * delta[i] ** 2)
        for k, (i, j) in enumerate(pairs):
            F[i, j] = F[j, i] = (c[1 + 2 * n + k] - c[1 + i] - c[1 + j] + c[0]) / (2 * delta[i] * delta[j])
        g = np.array([(c[1 + i] - c[0]) / delta[i] - F[i, i] * delta[i] for i in range(n)])
        return F, g

    F, _ = fit(np.ones(len(cols)))
    sd = 1.0 / np.sqrt(np.diag(F))
    F, g = fit(sd)
    cov = np.linalg.inv(F)
    mean = b0 - 0.5 * cov @ g
    chi2_min = float(chi2_at([mean - b0])[0])
    return names, mean, cov, F, float(auto_vega._log_norm()) - 0.5 * chi2_min


def test_merged_nested_replicas_give_the_exact_evidence(auto_vega):
    """Four linear broadband coefficients over b* +- 10 sd: log Z = lnL(b*) + 1/2 log|2 pi cov| - sum log(20 sd).  R = 4 at
    nlive 256 / K 64: |log Z - exact| <= 5 err, err within 10 % of the single runs' mean err / 2, weighted-mean pulls <= 5."""
    from vega_amd import NestedSampler
    from vega_amd import replicas as rep
    names, mean, cov, F, lnl_max = _linear_gaussian(auto_vega)
    sd = np.sqrt(np.diag(cov))
    log_z_true = lnl_max + 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1] - np.sum(np.log(20 * sd))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)}, 'values': dict(zip(names, mean)),
          'errors': dict(zip(names, sd))}
    runs = [NestedSampler(auto_vega, num_live=256, threads=64, seed=11, sample_params=sp, stream=r).run() for r in range(4)]
    assert all(s.terminated and s.driver == 'device' for s in runs)
    m = rep.merge_nested([rep.nested_record(s) for s in runs])
    single = np.array([s.log_evidence() for s in runs])
    ess = 1.0 / np.sum(m['weights']**2)
    got_mean = m['weights'] @ m['points']
    pulls = (got_mean - mean) / (sd / np.sqrt(ess))
    print(f'merged log Z {m["log_z"]:.4f} (true {log_z_true:.4f}, err {m["err"]:.4f}, pull {(m["log_z"] - log_z_true) / m["err"]:+.2f}), '
          f'single {np.round(single[:, 0], 4)} +- {np.round(single[:, 1], 4)}, mean err / 2 {single[:, 1].mean() / 2:.4f}, ESS {ess:.0f}, '
          f'mean pulls {np.round(pulls, 2)}, rows {[s.stats["rows"] for s in runs]}')
    assert abs(m['log_z'] - log_z_true) <= 5 * m['err']
    assert abs(m['err'] - single[:, 1].mean() / 2) <= 0.1 * single[:, 1].mean() / 2
    assert np.all(np.abs(pulls) <= 5), pulls
    assert m['num_live'] == 1024 and abs(m['weights'].sum() - 1.0) < 1e-12


def test_two_ensembles(tmp_path):
    from vega_amd import replicas as rep
    from vega_amd.ensemble import integrated_time
    config, folder = _config(tmp_path, 'ens', 'Ensemble', replicas=2, walkers='64', steps='400')
    out = _run(tmp_path, config)
    out.samplers[0].vega.close()
    assert {p.name for p in folder.iterdir() if p.suffix in FINAL} == {'run_1.txt', 'run_2.txt', 'run.paramnames', 'run.stats'}
    m = out.merged
    st = rep.read_stats(folder / 'run.stats')
    assert st['replicas'] == 2 and st['walkers'] == 64 and st['discard'] == 200
    rhat = np.array([st['Rhat'][nm] for nm in ('bias_eta_LYA', 'beta_LYA')])
    assert np.all(np.isfinite(rhat)) and np.array_equal(rhat, m['rhat'])
    for k in range(2):
        table = np.loadtxt(folder / f'run_{k + 1}.txt')
        assert table.shape == (400 * 64, 4) and np.array_equal(table[:, 2:], m['chains'][k].reshape(-1, 2))
    assert (folder / 'run.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
    kept = [c[200:] for c in m['chains']]

    def mean_and_se(chains):
        flat = np.concatenate([c.reshape(-1, 2) for c in chains])
        n_eff = sum(c.shape[0] * c.shape[1] / integrated_time(c) for c in chains)
        return flat.mean(axis=0), flat.std(axis=0) / np.sqrt(n_eff)

    pooled, se_pooled = mean_and_se(kept)
    first, se_first = mean_and_se(kept[:1])
    pulls = (pooled - first) / np.sqrt(se_pooled**2 + se_first**2)
    print(f'R-hat {rhat}, pooled {pooled} +- {se_pooled}, replica 0 {first} +- {se_first}, pulls {pulls}, acceptance {m["acceptance"]}')
    assert np.all(np.abs(pulls) <= 5), pulls
