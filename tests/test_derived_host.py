"""Derived parameters of the samplers, the parts that need no GPU: the chain writer with and without derived columns, the names,
labels and order of the marginalisation coefficients (reference vega/samplers/sampler_interface.py:82-89,
vega/vega_interface.py:371-383), the ``derived`` key of the three settings parsers, and a host statement of the fold the engine
builds at set-up (include/vegamx.h: vmx_marg_coeff_device): coeff = M (d - S DM x) = c0 - G dx."""
import configparser
import hashlib

import numpy as np
import pytest

from conftest import marginalization_problem, MARGINALIZATION_CASES


# ------------------------------------------------------------------ the fold, stated on the host
def fold_tensors(M, SX, d, x0):
    """What quad_build keeps per item: G = M (S DM) [n_templates, nq] and c0 = M r0, r0 = d - S DM x0 (float64, as the device)."""
    M, SX = np.asarray(M, dtype=np.float64), np.asarray(SX, dtype=np.float64)
    return M.dot(SX), M.dot(np.asarray(d, dtype=np.float64) - SX.dot(np.asarray(x0, dtype=np.float64)))


def folded_coeff(G, c0, dx):
    """coeff rows [B, n_templates] for walker rows dx [B, nq]."""
    return c0[None, :] - np.asarray(dx, dtype=np.float64).dot(G.T)


def direct_coeff_extended(M, SX, d, x):
    """M (d - S DM x) in extended precision."""
    L = np.longdouble
    return np.asarray(M, dtype=L).dot(np.asarray(d, dtype=L)[None, :].T - np.asarray(SX, dtype=L).dot(np.asarray(x, dtype=L).T)).T


def item_fold_inputs(item):
    """(M, S DM, d, x0) of a Problem item: the masked rows of its distortion matrix, its masked data vector, and a reference vector
    of the signal's size (the data vector on the model grid, gaps filled with zeros)."""
    n_model = item.model_grid.size if hasattr(item.model_grid, 'size') else len(item.model_grid)
    dm = item.distortion
    dense = np.eye(len(item.model_mask), n_model) if dm is None else (dm.toarray() if hasattr(dm, 'toarray') else np.asarray(dm))
    SX = np.asarray(dense, dtype=np.float64)[np.asarray(item.model_mask)]
    x0 = np.zeros(SX.shape[1])
    dv = np.nan_to_num(np.asarray(item.data_vec, dtype=np.float64))
    x0[:min(x0.size, dv.size)] = dv[:min(x0.size, dv.size)]
    return np.asarray(item.marg_diff2coeff, dtype=np.float64), SX, np.asarray(item.masked_data_vec, dtype=np.float64), x0


@pytest.mark.parametrize('case', sorted(MARGINALIZATION_CASES))
def test_the_fold_is_the_direct_map_to_rounding(tmp_path, case):
    """c0 - G dx against M (d - S DM (x0 + dx)) in np.longdouble for 16 seeded dx (2 % of the reference vector's size), bound
    1e-13 of the coefficients' scale (measured when the fold was proposed: <= 1.3e-15)."""
    prob = marginalization_problem(tmp_path, MARGINALIZATION_CASES[case])
    item = prob.items['lyalya_lyalya']
    M, SX, d, x0 = item_fold_inputs(item)
    assert M.shape == (item.marg_diff2coeff.shape[0], SX.shape[0]) and SX.shape[0] == d.size
    G, c0 = fold_tensors(M, SX, d, x0)
    rng = np.random.default_rng(11)
    dx = 0.02 * np.abs(x0).max() * rng.standard_normal((16, x0.size))
    got = folded_coeff(G, c0, dx)
    want = direct_coeff_extended(M, SX, d, x0[None, :] + dx)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f'{case}: templates {M.shape[0]}, |fold - direct| / scale = {err / scale:.3g}')
    assert err <= 1e-13 * scale


# ------------------------------------------------------------------ the chain writer
def _fixed_chain():
    rng = np.random.default_rng(5)
    return rng.standard_normal((6, 4, 2)), rng.standard_normal((6, 4))


def test_write_getdist_without_derived_arguments_is_what_it_was(tmp_path):
    """The bytes of both files for a fixed input, as the writer produced them before it took derived columns (np.savetxt
    '%.17g' of [1, -lnL, parameters]; 'name name' lines), and the explicit None arguments change nothing."""
    from vega_amd import ensemble as E
    chain, lnl = _fixed_chain()
    txt, pn = E.write_getdist(tmp_path, 'plain', ['x', 'y'], chain, lnl)
    rows = np.column_stack([np.ones(24), -lnl.reshape(-1), chain.reshape(-1, 2)])
    want = ''.join(' '.join('%.17g' % v for v in row) + '\n' for row in rows)
    assert txt.read_text() == want
    assert pn.read_text() == 'x x\ny y\n'
    txt2, pn2 = E.write_getdist(tmp_path, 'none', ['x', 'y'], chain, lnl, derived=None, derived_names=None, derived_labels=None)
    assert txt2.read_bytes() == txt.read_bytes() and pn2.read_bytes() == pn.read_bytes()
    assert hashlib.sha256(txt.read_bytes()).hexdigest() == hashlib.sha256(want.encode()).hexdigest()


def test_write_getdist_with_derived_columns(tmp_path):
    from vega_amd import ensemble as E
    chain, lnl = _fixed_chain()
    derived = np.random.default_rng(6).standard_normal((6, 4, 3))
    names, labels = E.marg_derived_labels({'b': 2, 'a': 1})
    txt, pn = E.write_getdist(tmp_path, 'd', ['x', 'y'], chain, lnl, derived=derived, derived_names=names, derived_labels=labels)
    table = np.loadtxt(txt)
    assert table.shape == (24, 2 + 2 + 3)
    np.testing.assert_array_equal(table[:, :4], np.loadtxt(E.write_getdist(tmp_path, 'p', ['x', 'y'], chain, lnl)[0]))
    np.testing.assert_array_equal(table[:, 4:], derived.reshape(-1, 3))
    assert pn.read_text().splitlines() == ['x x', 'y y', r'a_marg_0 M_{\rm a}^{0}', r'b_marg_0 M_{\rm b}^{0}', r'b_marg_1 M_{\rm b}^{1}']
    # weights and derived columns together (a nested run)
    w = np.full((6, 4), 0.25)
    table_w = np.loadtxt(E.write_getdist(tmp_path, 'w', ['x', 'y'], chain, lnl, weights=w, derived=derived, derived_names=names)[0])
    assert np.all(table_w[:, 0] == 0.25) and np.array_equal(table_w[:, 1:], table[:, 1:])
    assert (tmp_path / 'w.paramnames').read_text().splitlines()[2:] == [f'{n} {n}' for n in names]
    with pytest.raises(ValueError):
        E.write_getdist(tmp_path, 'bad', ['x', 'y'], chain, lnl, derived=derived)
    with pytest.raises(ValueError):
        E.write_getdist(tmp_path, 'bad', ['x', 'y'], chain, lnl, derived=derived[:5], derived_names=names)


def test_names_labels_and_sorted_correlation_order():
    from vega_amd import ensemble as E
    names, labels = E.marg_derived_labels({'qsoxlya': 2, 'lyaxlya': 3})
    assert names == ['lyaxlya_marg_0', 'lyaxlya_marg_1', 'lyaxlya_marg_2', 'qsoxlya_marg_0', 'qsoxlya_marg_1']
    assert labels == [r'M_{\rm lyaxlya}^{0}', r'M_{\rm lyaxlya}^{1}', r'M_{\rm lyaxlya}^{2}', r'M_{\rm qsoxlya}^{0}',
                      r'M_{\rm qsoxlya}^{1}']
    assert E.marg_derived_labels({}) == ([], [])


def test_derived_names_of_an_interface_follow_the_returned_vector(tmp_path):
    """``VegaInterface.derived_names`` is a function of the problem alone: sorted correlations, ``marg_diff2coeff.shape[0]``
    coefficients each (class-level: no engine)."""
    from types import SimpleNamespace
    from vega_amd.interface import VegaInterface
    items = {'zz': SimpleNamespace(marg_diff2coeff=np.zeros((2, 5))), 'mm': SimpleNamespace(marg_diff2coeff=None),
             'aa': SimpleNamespace(marg_diff2coeff=np.zeros((3, 7)))}
    fake = SimpleNamespace(problem=SimpleNamespace(items=items), _marg_names=['zz', 'aa'])
    assert VegaInterface.derived_names(fake) == ['aa_marg_0', 'aa_marg_1', 'aa_marg_2', 'zz_marg_0', 'zz_marg_1']
    assert VegaInterface.derived_labels(fake) == [r'M_{\rm aa}^{0}', r'M_{\rm aa}^{1}', r'M_{\rm aa}^{2}', r'M_{\rm zz}^{0}',
                                                  r'M_{\rm zz}^{1}']
    fake._marg_names = []
    assert VegaInterface.derived_names(fake) == []


# ------------------------------------------------------------------ the settings parsers
def _config(tmp_path, sampler, extra):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg['control'] = {'run_sampler': 'True', 'sampler': sampler}
    cfg[sampler] = dict({'path': str(tmp_path)}, **extra)
    return cfg


@pytest.mark.parametrize('sampler', ['Ensemble', 'Nested', 'SMC'])
def test_settings_parsers_read_the_derived_key(tmp_path, sampler):
    from vega_amd.ensemble import sampler_settings
    sp = {'limits': {'ap': (0.5, 1.5), 'at': (0.5, 1.5)}}
    # (absent: the settings are the dictionary they were - the existing tests pin it - and the option reads as False)
    assert sampler_settings(_config(tmp_path, sampler, {}), sp).get('derived', False) is False
    assert sampler_settings(_config(tmp_path, sampler, {'derived': 'True'}), sp)['derived'] is True
    assert sampler_settings(_config(tmp_path, sampler, {'derived': 'False'}), sp)['derived'] is False
    with pytest.raises(ValueError, match='derived'):
        sampler_settings(_config(tmp_path, sampler, {'derived': 'sometimes'}), sp)
