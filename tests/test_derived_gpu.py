"""Marginalisation coefficients as derived columns of the device samplers (include/vegamx.h: vmx_marg_coeff_device): the
coefficients of walkers that live in HBM from the chi2 path's own walker vectors through the map folded at set-up
(coeff = c0 - G dx), against the reference's fixture, against the full-chain route ``chi2_batch(return_marg_coeff=True)``,
in Monte-Carlo mode, for the three template configurations, and through the three samplers and the config switch."""
import configparser

import numpy as np
import pytest

from conftest import GOLDEN, marginalization_problem, MARGINALIZATION_CASES
from test_derived_host import fold_tensors, folded_coeff, item_fold_inputs

pytestmark = pytest.mark.gpu

NAME = 'lyalya_lyalya'


def _device_block(vega, theta):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(theta))).to(torch.device('cuda', getattr(vega.engine, 'device', 0)))
    out = vega.marg_coeff_batch_device(t)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (t.shape[0], len(vega.derived_names()))
    return out.cpu().numpy()


def _numpy_map(vega, item, theta_row):
    """M . (masked data - model[mask]) with the engine's own full-chain model."""
    _, status, model = vega.engine.eval(np.atleast_2d(theta_row), want_model=True)
    assert not status.any()
    return item.marg_diff2coeff.dot(item.masked_data_vec - model[0, vega.engine.model_slices[NAME]][item.model_mask])


def _report(what, got, want):
    scale = float(np.abs(want).max())
    err = float(np.nanmax(np.abs(got - want)))
    print(f'{what}: max |diff| / scale = {err / scale:.3g}')
    return err, scale


def _walkers(vega, prob, n, seed):
    from vega_amd import synthetic
    eng = vega.engine
    limits = {k: tuple(v) for k, v in prob.sample_params['limits'].items()}
    return synthetic.walkers(eng.low.theta0, eng.names, n, varied=list(limits), seed=seed, limits=limits)


@pytest.fixture(scope='module')
def rtmax(tmp_path_factory):
    from vega_amd import VegaInterface
    prob = marginalization_problem(tmp_path_factory.mktemp('rtmax'), MARGINALIZATION_CASES['rtmax'])
    vega = VegaInterface(None, problem=prob, max_batch=16)
    yield vega, prob
    vega.close()


@pytest.mark.parametrize('mode', ['cov', 'infit'])
def test_reference_fixture(tmp_path, mode):
    """1. The fiducial point and walker 0 of the reference's fixture: 5e-6 of the scale against the fixture (the host dependence
    of the reference's inv(A) . G, as tests/test_round2_gpu.py), 1e-10 against the same map applied by NumPy."""
    from vega_amd import VegaInterface
    exp = np.load(GOLDEN / 'expected_marg_coeff.npz')
    prob = marginalization_problem(tmp_path, MARGINALIZATION_CASES['rtmax'], in_fit=mode == 'infit')
    item = prob.items[NAME]
    vega = VegaInterface(None, problem=prob, max_batch=16)
    try:
        assert vega.engine.quadratic_form
        assert vega.derived_names() == [f'{NAME}_marg_{i}' for i in range(item.marg_diff2coeff.shape[0])]
        pars = {str(n): float(v) for n, v in zip(exp[f'{mode}/param_names'], exp[f'{mode}/theta'][0])}
        for tag, theta in (('fid', vega._theta()), ('walker0', vega._theta(pars))):
            got = _device_block(vega, theta)[0]
            assert vega.engine.last_form() in ('q', 'factored')
            ref = exp[f'{mode}/{tag}/coeff']
            err, scale = _report(f'{mode} {tag} against the fixture', got, ref)
            assert err <= 5e-6 * scale
            want = _numpy_map(vega, item, theta)
            err, scale = _report(f'{mode} {tag} against NumPy on the engine model', got, want)
            assert err <= 1e-10 * scale
    finally:
        vega.close()


def test_the_chi2_path_served_it(rtmax):
    """2. The form is on, the call took it ('q' / 'factored', never 'full'), both forms give the same block, and with the form
    switched off the same entry takes the full chain and gives the same block."""
    vega, prob = rtmax
    eng = vega.engine
    assert eng.quadratic_form
    theta = _walkers(vega, prob, 16, seed=2)
    blocks = {}
    try:
        for kind in ('q', 'factored'):
            eng.set_quadratic_form_kind(kind)
            blocks[kind] = _device_block(vega, theta)
            assert eng.last_form() == kind
        err, scale = _report('q against factored', blocks['q'], blocks['factored'])
        assert np.isfinite(blocks['q']).all() and err <= 1e-12 * scale
        eng.set_quadratic_form_kind('auto')
        auto = _device_block(vega, theta)
        assert eng.last_form() in ('q', 'factored')
        eng.set_quadratic_form(False)
        full = _device_block(vega, theta)
        assert eng.last_form() == 'full'
        err, scale = _report('folded against the full-chain fallback', auto, full)
        assert err <= 1e-10 * scale
    finally:
        eng.set_quadratic_form_kind('auto')
        assert eng.set_quadratic_form(True)


def test_batches(rtmax):
    """3. 64 walkers in four chunks of max_batch = 16 against the host route; a failing walker in the middle of a chunk is NaN in
    all its columns and leaves its neighbours' rows alone; the call is deterministic."""
    vega, prob = rtmax
    theta = _walkers(vega, prob, 64, seed=3)
    got = _device_block(vega, theta)
    assert vega.engine.last_form() in ('q', 'factored')
    want = vega.chi2_batch(theta, return_marg_coeff=True)[1][NAME]
    assert np.isfinite(want).all()
    err, scale = _report('64 walkers against chi2_batch(return_marg_coeff=True)', got, want)
    assert err <= 1e-10 * scale
    again = _device_block(vega, theta)
    assert np.array_equal(got, again)
    bad = theta.copy()
    bad[21, vega.engine.low.slot['ap']] = 1e3
    with_bad = _device_block(vega, bad)
    assert np.isnan(with_bad[21]).all()
    keep = np.arange(64) != 21
    assert np.isfinite(with_bad[keep]).all()
    print('neighbours of the failing walker bit for bit:', bool(np.array_equal(with_bad[keep], got[keep])))
    assert np.abs(with_bad[keep] - got[keep]).max() <= 1e-12 * scale
    # ... as the host route marks it
    assert np.isnan(vega.chi2_batch(bad[16:32], return_marg_coeff=True)[1][NAME][5]).all()


def test_monte_carlo_mode(tmp_path):
    """4. The call sequence of test_rescaled_covariance_with_marginalize_in_fit_through_the_engine: with the mock installed the
    block is the reference's; with a pool of 8 mocks and a per-walker index row b is the single-mock answer of mock(b).
    (The pool's constants c0 = M r0 come from one product over 9 rows, a single mock's from a product over one: other kernels of
    the same engine, so equal to the rounding of a 1590-term fp64 sum with the map's tenfold cancellation, ~1e-14 of the scale;
    the bound is 1e-12.)"""
    from vega_amd import VegaInterface
    exp = np.load(GOLDEN / 'expected_marg_mc.npz')
    prob = marginalization_problem(tmp_path, MARGINALIZATION_CASES['rtmax'], in_fit=True)
    item = prob.items[NAME]
    vega = VegaInterface(None, problem=prob, max_batch=16)
    try:
        eng = vega.engine
        assert eng.quadratic_form
        plain = _device_block(vega, vega._theta())
        view = vega.data[NAME]
        view.masked_mc_mock = exp['mock']
        view.scaled_inv_masked_cov = view.inv_masked_cov / float(exp['scale'])
        vega.monte_carlo = True
        got = _device_block(vega, vega._theta())[0]
        assert eng.last_form() in ('q', 'factored')
        err, scale = _report('mock installed, against the fixture', got, exp['fid/coeff'])
        assert err <= 5e-6 * scale
        host = vega.chi2(return_marg_coeff=True)[1][NAME]
        assert np.abs(got - host).max() <= 1e-10 * scale
        vega.monte_carlo = False
        back = _device_block(vega, vega._theta())
        assert np.abs(back - plain).max() <= 1e-12 * np.abs(plain).max()
        # a pool of 8 mocks, the walkers of one batch on different rows of it (and some on the data vector)
        rng = np.random.default_rng(8)
        sigma = float(np.std(np.asarray(exp['mock']) - np.asarray(item.masked_data_vec)))         # the mock's own noise level
        mocks = np.asarray(exp['mock'])[None, :] + sigma * rng.standard_normal((8, exp['mock'].size))
        theta = _walkers(vega, prob, 16, seed=4)
        index = np.array([0, 1, 2, 3, 4, 5, 6, 7, -1, 7, 3, -1, 0, 5, 2, 6], dtype=np.int32)
        single = {-1: _device_block(vega, theta)}
        for k in range(8):
            eng.set_data(NAME, mocks[k])
            single[k] = _device_block(vega, theta)
        eng.set_data(NAME, item.masked_data_vec)
        eng.set_mock_pool(NAME, mocks)
        eng.set_mock_index(index)
        pooled = _device_block(vega, theta)
        assert eng.last_form() in ('q', 'factored')
        eng.set_mock_index(None)
        want = np.stack([single[int(k)][b] for b, k in enumerate(index)])
        err, scale = _report('pool of 8 mocks, per-walker rows', pooled, want)
        assert err <= 1e-12 * scale
        assert np.abs(single[0] - single[1]).max() > 1e-3 * scale          # (the mocks do differ)
        after = _device_block(vega, theta)
        assert np.abs(after - single[-1]).max() <= 1e-12 * scale
    finally:
        vega.close()


@pytest.mark.parametrize('case', ['allrmin', 'fitscales'])
def test_all_cases_build(tmp_path, case):
    """5. 4 templates (the small-batch product kernels) and 150 with their own masks, against the NumPy map."""
    from vega_amd import VegaInterface
    prob = marginalization_problem(tmp_path, MARGINALIZATION_CASES[case])
    item = prob.items[NAME]
    vega = VegaInterface(None, problem=prob, max_batch=16)
    try:
        assert vega.engine.quadratic_form
        assert len(vega.derived_names()) == item.marg_diff2coeff.shape[0]
        theta = _walkers(vega, prob, 16, seed=5)
        theta[0] = vega._theta()
        got = _device_block(vega, theta)
        assert vega.engine.last_form() in ('q', 'factored')
        for b in (0, 1, 15):
            want = _numpy_map(vega, item, theta[b])
            err, scale = _report(f'{case} walker {b} against NumPy on the engine model', got[b], want)
            assert err <= 1e-10 * scale
        # the host statement of the fold reproduces its own direct map on this item (what the device builds, in NumPy)
        M, SX, d, x0 = item_fold_inputs(item)
        G, c0 = fold_tensors(M, SX, d, x0)
        assert np.abs(folded_coeff(G, c0, np.zeros((1, x0.size)))[0] - M.dot(d - SX.dot(x0))).max() <= 1e-13 * np.abs(c0).max()
    finally:
        vega.close()


@pytest.mark.parametrize('variant', ['reversed_items', 'global_covariance'])
def test_two_correlations_layout_and_the_global_covariance_fallback(variant):
    """Two correlations with (seeded, arbitrary) maps of different sizes on the synthetic joint problem: the columns come sorted
    by correlation name whatever the engine's item order ('reversed_items': the engine holds them in reverse, the block is
    permuted on the device), and under a global covariance - which the quadratic form does not serve - the same call takes the
    full chain ('full') and gives what the host route gives."""
    from conftest import synth_joint_problem
    from vega_amd import VegaInterface, synthetic
    prob = synth_joint_problem(with_global_cov=variant == 'global_covariance')
    rng = np.random.default_rng(12)
    for i, item in enumerate(prob.items.values()):
        item.marg_diff2coeff = rng.standard_normal((3 + 2 * i, item.masked_data_vec.size))
    if variant == 'reversed_items':
        prob.items = dict(reversed(list(prob.items.items())))
    vega = VegaInterface(None, problem=prob, max_batch=16)
    try:
        eng = vega.engine
        assert bool(eng.quadratic_form) == (variant != 'global_covariance')
        names = sorted(prob.items)
        assert vega.derived_names() == [f'{n}_marg_{i}' for n in names for i in range(prob.items[n].marg_diff2coeff.shape[0])]
        if variant == 'reversed_items':
            assert list(eng.item_names) == names[::-1]
        theta = synthetic.walkers(eng.low.theta0, eng.names, 16, varied=['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO'], seed=6)
        got = _device_block(vega, theta)
        assert (eng.last_form() == 'full') == (variant == 'global_covariance')
        coeff = vega.chi2_batch(theta, return_marg_coeff=True)[1]
        want = np.hstack([coeff[n] for n in names])
        err, scale = _report(f'{variant}: two correlations against the host route', got, want)
        assert np.isfinite(got).all() and err <= 1e-10 * scale
    finally:
        vega.close()


# ------------------------------------------------------------------ 6. the samplers
@pytest.fixture(scope='module')
def rtmax64(tmp_path_factory):
    from vega_amd import VegaInterface
    prob = marginalization_problem(tmp_path_factory.mktemp('rtmax64'), MARGINALIZATION_CASES['rtmax'])
    vega = VegaInterface(None, problem=prob, max_batch=64)
    yield vega, prob
    vega.close()


def _check_derived(vega, sampler, rows, block):
    n_derived = len(vega.derived_names())
    assert n_derived == 200 and block.shape == (rows.shape[0], n_derived)
    theta = np.repeat(np.asarray(vega._theta(None))[None, :], rows.shape[0], axis=0)
    theta[:, sampler.cols] = rows
    want = vega.chi2_batch(theta, return_marg_coeff=True)[1][NAME]
    err, scale = _report(f'{type(sampler).__name__} ({sampler.driver}): derived block against the host route', block, want)
    assert np.isfinite(block).all() and err <= 1e-10 * scale


def test_ensemble_sampler_derived(rtmax64):
    from vega_amd import EnsembleSampler
    vega, prob = rtmax64
    blocks = []
    for driver in ('device', 'python'):
        s = EnsembleSampler(vega, 32, seed=5, driver=driver).run(20)
        assert s.driver == driver
        block = s.get_derived()
        assert block.shape == (20, 32, 200)
        flat = s.get_derived(flat=True)
        assert np.array_equal(flat, block.reshape(-1, 200))
        _check_derived(vega, s, s.get_chain(flat=True), flat)
        assert s.get_derived(discard=4, thin=2).shape == (8, 32, 200)
        plain = EnsembleSampler(vega, 32, seed=5, driver=driver).run(20)
        assert np.array_equal(plain.get_chain(), s.get_chain()) and np.array_equal(plain.get_log_lik(), s.get_log_lik())
        blocks.append(flat)
    assert np.array_equal(blocks[0], blocks[1])


def test_nested_sampler_derived(rtmax64):
    from vega_amd import NestedSampler
    vega, prob = rtmax64
    blocks = []
    for driver in ('device', 'python'):
        s = NestedSampler(vega, num_live=64, seed=5, driver=driver)
        s.run(iterations=3)
        assert s.driver == driver
        pts, lnl, _ = s.samples()
        block = s.derived()
        assert block.shape[0] == pts.shape[0] == lnl.size
        _check_derived(vega, s, pts, block)
        plain = NestedSampler(vega, num_live=64, seed=5, driver=driver)
        plain.run(iterations=3)
        assert np.array_equal(plain.samples()[0], pts) and np.array_equal(plain.samples()[1], lnl)
        blocks.append(block)
    assert np.array_equal(blocks[0], blocks[1])


def test_smc_sampler_derived(rtmax64):
    from vega_amd import SMCSampler
    vega, prob = rtmax64
    blocks = []
    for driver in ('device', 'python'):
        s = SMCSampler(vega, particles=256, seed=5, driver=driver)
        s.run(stages=2)
        assert s.driver == driver
        pts, lnl, _ = s.samples()
        block = s.derived()
        assert block.shape[0] == pts.shape[0] == 256
        _check_derived(vega, s, pts, block)
        plain = SMCSampler(vega, particles=256, seed=5, driver=driver)
        plain.run(stages=2)
        assert np.array_equal(plain.samples()[0], pts) and np.array_equal(plain.samples()[1], lnl)
        blocks.append(block)
    assert np.array_equal(blocks[0], blocks[1])


def _sampler_config(tmp_path, tag, extra):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / 'configs' / 'marg' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Ensemble'
    out = tmp_path / f'chains_{tag}'
    out.mkdir()
    cfg['Ensemble'] = dict({'path': str(out), 'name': 'chain', 'walkers': '8', 'steps': '12', 'thin': '3', 'seed': '4'}, **extra)
    (tmp_path / 'configs' / tag).mkdir(parents=True)
    with open(tmp_path / 'configs' / tag / 'main.ini', 'w') as f:
        cfg.write(f)
    return f'configs/{tag}/main.ini', out


def test_run_vega_sampler_with_the_derived_key(tmp_path):
    from vega_amd import run_vega_sampler
    prob = marginalization_problem(tmp_path, MARGINALIZATION_CASES['rtmax'])
    sampled = list(prob.sample_params['limits'])
    files = {}
    for tag, extra in (('on', {'derived': 'True'}), ('absent', {}), ('off', {'derived': 'False'})):
        main, out = _sampler_config(tmp_path, tag, extra)
        sampler = run_vega_sampler(main, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None, max_batch=16)
        files[tag] = ((out / 'chain.txt').read_bytes(), (out / 'chain.paramnames').read_bytes())
        table = np.loadtxt(out / 'chain.txt')
        lines = (out / 'chain.paramnames').read_text().splitlines()
        if tag == 'on':
            names, labels = sampler.vega.derived_names(), sampler.vega.derived_labels()
            assert len(names) == 200 and names[0] == f'{NAME}_marg_0' and labels[3] == r'M_{\rm ' + NAME + '}^{3}'
            assert table.shape == (12 // 3 * 8, 2 + len(sampled) + len(names))
            assert lines == [f'{n} {n}' for n in sampled] + [f'{n} {l}' for n, l in zip(names, labels)]
            np.testing.assert_array_equal(table[:, 2 + len(sampled):], sampler.get_derived(flat=True))
            np.testing.assert_array_equal(table[:, 2:2 + len(sampled)], sampler.get_chain(flat=True))
        else:
            assert table.shape == (12 // 3 * 8, 2 + len(sampled))
            assert lines == [f'{n} {n}' for n in sampled]
        sampler.vega.close()
    assert files['absent'] == files['off']
    assert files['on'][0] != files['off'][0]


def test_derived_without_templates_writes_the_plain_chain(tmp_path):
    """``derived = True`` on a configuration without templates: the plain chain and a line through print_func."""
    from vega_amd import EnsembleSampler, VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=16)
    try:
        assert vega.derived_names() == []
        s = EnsembleSampler(vega, 8, seed=1).run(3)
        said = []
        s.write(tmp_path, 'with', derived=True, print_func=said.append)
        s.write(tmp_path, 'without')
        assert len(said) == 1 and 'templates' in said[0]
        assert (tmp_path / 'with.txt').read_bytes() == (tmp_path / 'without.txt').read_bytes()
        assert (tmp_path / 'with.paramnames').read_bytes() == (tmp_path / 'without.paramnames').read_bytes()
        assert s.get_derived(flat=True).shape == (24, 0)
    finally:
        vega.close()
