"""Small, awkward correlation grids for tests/test_grid_shapes_gpu.py and tests/golden/make_golden.py::dump_small_grids.

Every case is a set of correlations on grids of 4 Mpc/h bins built by vega_amd.synthetic.grid_tables, written in the
reference's file layout (synthetic.write_data_file, synthetic.write_dmat_file_case) and read back through build_problem:
the sizes at which the products after xi change their tiling (one 64-row tile, one row more, odd and even remainders, exact
multiples, K above the single-walker kernels' limits, a one-tile item next to a 21-tile item on one launch).

Each case states what it reaches next to its definition (``facts``); `check_facts` holds a built Problem to them, so a
change of cuts cannot quietly empty the coverage.
"""
import re
from pathlib import Path

import numpy as np

BIN = 4.0
POST_ADD_TERM = 'bb1 = add post r,mu 0:2:1 0:6:2'      # the golden auto config's broadband: 3 x 4 = 12 coefficients
N_POST_ADD = 12
WALKER_SEED = 20260803 + 29
N_WALKERS = 3           # + the fiducial point: four parameter rows per case


def tape_row0(nq, bm=64):
    """vmx_plan::tape_row0: an even remainder is the first, ragged row tile of the Q' tape; an odd one (or none) tiles
    from row 0 and leaves the ragged tile last."""
    r = nq % bm
    return r if r % 2 == 0 else 0


def _item(kind, n_p, n_t, r_min=10., r_max=180., coef=1, broadband=False, z_scatter=0.0):
    return dict(kind=kind, n_p=n_p, n_t=n_t, r_min=r_min, r_max=r_max, coef=coef, broadband=broadband, z_scatter=z_scatter)


def _facts(n_model, nq, n_masked):
    """Per item: the sizes, their remainders, the Q' tape's first-tile rows and the row-tile counts."""
    return [dict(n_model=m, nq=q, n_masked=k, nq_mod64=q % 64, n_model_mod4=m % 4, n_masked_mod64=k % 64,
                 n_masked_mod4=k % 4, row0=tape_row0(q), row_tiles=-(-q // 64), masked_tiles=-(-k // 64))
            for m, q, k in zip(n_model, nq, n_masked)]


# name -> (items, claimed facts).  The literal numbers are claims: check_facts compares them with the built Problem.
CASES = {
    # less than one tile everywhere, tm = 1, 63 % 4 = 3
    'a63': ([_item('auto', 7, 9)], _facts([63], [63], [59])),
    # exactly one tile
    'a64': ([_item('auto', 8, 8)], _facts([64], [64], [60])),
    # one row into the second tile, odd remainder 1; no r cut: the C^-1 products have the same one-row second tile
    'a65': ([_item('auto', 5, 13, r_min=0.)], _facts([65], [65], [65])),
    # ... and with cuts that leave less than one tile of masked bins
    'a65_cut': ([_item('auto', 5, 13, r_min=10., r_max=40.)], _facts([65], [65], [44])),
    # odd remainder 63, pad 1024
    'a1023': ([_item('auto', 31, 33)], _facts([1023], [1023], [1019])),
    # remainder 0 (the one case whose n_masked is a multiple of 64)
    'a1024': ([_item('auto', 32, 32, r_min=0.)], _facts([1024], [1024], [1024])),
    # odd remainder 7, 21 row tiles
    'a1287': ([_item('auto', 33, 39)], _facts([1287], [1287], [1243])),
    # ... with the additive polynomial post-distortion broadband: nq = n_model + 12, remainder 19
    'a1287_bb': ([_item('auto', 33, 39, broadband=True)], _facts([1287], [1299], [1243])),
    # even remainder 16: the tape's first tile has 16 rows
    'a1296': ([_item('auto', 36, 36, r_max=140.)], _facts([1296], [1296], [959])),
    # a one-tile item and a 21-tile item on one tape and in one grouped launch
    'j_small_big': ([_item('auto', 7, 9), _item('cross', 40, 33, z_scatter=0.02)],
                    _facts([63, 1320], [63, 1320], [59, 1312])),
    # K above 2560 (k_gemv1<10, .>), row0 = 32
    'j_2592': ([_item('auto', 36, 36), _item('cross', 72, 36, z_scatter=0.02)],
               _facts([1296, 2592], [1296, 2592], [1256, 2512])),
    # data 36 x 36, model 72 x 72 (COEFMOD 2): K above 5120 - a single walker leaves k_gemv1; the factored form
    'r5184': ([_item('auto', 36, 36, coef=2)], _facts([5184], [5184], [1256])),
}
# what the literal claims above must amount to (the table of the cases: checked without a GPU by check_claims)
EXPECTED_REMAINDERS = {'a63': [(63, 0)], 'a64': [(0, 0)], 'a65': [(1, 0)], 'a65_cut': [(1, 0)], 'a1023': [(63, 0)],
                       'a1024': [(0, 0)], 'a1287': [(7, 0)], 'a1287_bb': [(19, 0)], 'a1296': [(16, 16)],
                       'j_small_big': [(63, 0), (40, 40)], 'j_2592': [(16, 16), (32, 32)], 'r5184': [(0, 0)]}
ITEM_FILES = {'auto': ('auto', 'lyalya_lyalya'), 'cross': ('joint', 'lyalya_qso')}


def check_claims():
    """The cases together: (nq mod 64, tape_row0) per item as the table states them; n_masked odd at least twice, a multiple
    of 64 at most once, ceil(n_masked / 64) of both parities; a row-tile count of 1 next to one of 21."""
    masked = []
    for name, (items, facts) in CASES.items():
        assert [(f['nq_mod64'], f['row0']) for f in facts] == EXPECTED_REMAINDERS[name], name
        masked += [f['n_masked'] for f in facts]
    assert sum(k % 2 for k in masked) >= 2
    assert sum(k % 64 == 0 for k in set(masked)) <= 1
    assert {-(-k // 64) % 2 for k in masked} == {0, 1}
    assert any(k < 64 for k in masked)
    assert [f['row_tiles'] for f in CASES['j_small_big'][1]] == [1, 21]
    assert CASES['a1287'][1][0]['row_tiles'] == 21 and CASES['a63'][1][0]['n_model_mod4'] == 3
    assert CASES['j_2592'][1][1]['nq'] > 2560 and CASES['r5184'][1][0]['nq'] > 5120
    check_metal_claims()


def item_geometry(item):
    """(rp_min, rp_max, rt_max, NP, NT) of the DATA grid: auto-correlations have rp from 0, crosses are symmetric in rp."""
    n_p, n_t = item['n_p'], item['n_t']
    if item['kind'] == 'auto':
        return 0., BIN * n_p, BIN * n_t, n_p, n_t
    return -BIN * n_p / 2, BIN * n_p / 2, BIN * n_t, n_p, n_t


def item_tables(item):
    from vega_amd import synthetic
    return synthetic.grid_tables(*item_geometry(item), z=2.3, z_scatter=item['z_scatter'])


def write_item_files(directory, item, tag):
    """The data file (+ distortion and covariance files for COEFMOD 2) of one item; returns the [data] lines that name them."""
    from vega_amd import synthetic
    directory = Path(directory)
    source = item_tables(item)
    if item['coef'] == 1:
        # (new_metals builds its matrices with the cosmology of the data file's header)
        extra = synthetic.PICCA_COSMOLOGY_HEADER if item.get('metals') else None
        path = synthetic.write_data_file(directory / f'{tag}.fits', source, extra_header=extra)
        return f'filename = {path}'
    path = synthetic.write_data_file(directory / f'{tag}.fits', source, with_distortion=False, with_covariance=False)
    sub = directory / f'{tag}_dmat'
    sub.mkdir(exist_ok=True)
    dmat, cov = synthetic.write_dmat_file_case(sub, source, coef=item['coef'])
    return f'filename = {path}\ndistortion-file = {dmat}\ncovariance-file = {cov}'


def adapt_item_ini(text, item, data_lines):
    """An item's ini text with its file names replaced, the r cuts adapted to the grid (everything else stays as wide as
    the golden config has it) and the broadband section kept only where the case asks for it."""
    text = re.sub(r'filename = .*', lambda _: data_lines, text, count=1)
    text = re.sub(r'r-min = .*', f'r-min = {item["r_min"]}', text, count=1)
    text = re.sub(r'r-max = .*', f'r-max = {item["r_max"]}', text, count=1)
    text = re.sub(r'\[broadband\][^\[]*', '', text)
    if not item.get('metals'):
        text = re.sub(r'\[metals\][^\[]*', '', text)
    if item['broadband']:
        text = text.rstrip('\n') + f'\n\n[broadband]\n{POST_ADD_TERM}\n'
    return text


def write_case(tmp_path, case, golden):
    """The files and ini files of ``case`` under ``tmp_path``, starting from tests/golden/configs/auto and configs/joint;
    returns the main file's path relative to ``tmp_path`` (a search directory for build_problem)."""
    tmp_path, golden = Path(tmp_path), Path(golden)
    if case in METAL_CASES:
        return write_metal_case(tmp_path, case, golden)
    items, _ = CASES[case]
    cfg = tmp_path / 'configs' / case
    cfg.mkdir(parents=True, exist_ok=True)
    main = (golden / 'configs' / ('auto' if len(items) == 1 else 'joint') / 'main.ini').read_text()
    names = []
    for i, item in enumerate(items):
        config, name = ITEM_FILES[item['kind']]
        text = (golden / 'configs' / config / f'{name}.ini').read_text()
        (cfg / f'{name}.ini').write_text(adapt_item_ini(text, item, write_item_files(tmp_path, item, f'{case}_{i}')))
        names.append(name)
    main = re.sub(r'ini files = .*', 'ini files = ' + ' '.join(f'configs/{case}/{n}.ini' for n in names), main)
    (cfg / 'main.ini').write_text(main)
    return f'configs/{case}/main.ini'


def build_case(tmp_path, case, golden):
    from vega_amd.setup import build_problem
    return build_problem(write_case(tmp_path, case, golden), search_dirs=[tmp_path, golden])


def check_facts(case, problem):
    """The built Problem against the case's claims (before anything runs on a device)."""
    if case in METAL_CASES:
        return check_metal_facts(case, problem)
    items, facts = CASES[case]
    assert len(problem.items) == len(items)
    for item, fact, got in zip(items, facts, problem.items.values()):
        n_post = sum(len(np.arange(t.r1[0], t.r1[1] + 1, t.r1[2])) * len(np.arange(t.r2[0], t.r2[1] + 1, t.r2[2]))
                     for t in got.broadband if (t.pos, t.kind) == ('post', 'add') and t.func != 'broadband_sky')
        assert n_post == (N_POST_ADD if item['broadband'] else 0)
        nq, n_model, n_masked = got.model_grid.size + n_post, got.model_grid.size, int(got.model_mask.sum())
        assert (n_model, nq, n_masked) == (fact['n_model'], fact['nq'], fact['n_masked']), (case, n_model, nq, n_masked)
        assert got.dist_grid.size == item['n_p'] * item['n_t'] and n_model == got.dist_grid.size * item['coef']**2
        assert got.data_size == n_masked and got.distortion.shape == (got.dist_grid.size, n_model)
        assert (nq % 64, n_model % 4, n_masked % 64, n_masked % 4) == \
            (fact['nq_mod64'], fact['n_model_mod4'], fact['n_masked_mod64'], fact['n_masked_mod4'])
        assert (tape_row0(nq), -(-nq // 64), -(-n_masked // 64)) == (fact['row0'], fact['row_tiles'], fact['masked_tiles'])


# ---------------------------------------------------------------------------------------------------------------------
# The metal terms on the same kind of grid (tests/test_metal_shapes_gpu.py, tests/golden/make_golden.py::dump_small_metals):
# `new_metals = True` builds every pair's matrix at set-up from a stacked-delta file and an object catalogue
# (vega_amd.synthetic), as a Kronecker product A [n_rp^2] (x) B [n_rt^2] - or A alone with `rp_only_metal_mats` - on any grid.
# k_metal_kron gives a thread five consecutive outputs on both axes: the cases cover every remainder of n_rp and n_rt mod 5.
# ---------------------------------------------------------------------------------------------------------------------
KRON_LDS_BYTES = 160 * 1024         # vmx_item_set_metal_kron: Xi, T and the larger factor in LDS
N_METAL_PAIRS = {'auto': (15, 4, 11), 'cross': (4, 4, 0)}       # pairs, of those with the main tracer, metal x metal
METAL_ITEM_FILES = {'auto': ('auto_metals', 'lyalya_lyalya'), 'cross': ('joint_metals', 'lyalya_qso')}


def _metal_item(kind, n_p, n_t, r_min=10., r_max=180., rp_only=False, z_scatter=0.0):
    return dict(_item(kind, n_p, n_t, r_min=r_min, r_max=r_max, z_scatter=z_scatter), metals=True, rp_only=rp_only)


def _metal_facts(items, n_masked):
    """Per item: the sizes, the pair counts and the Kronecker factor sizes (n_rp, n_rt; n_rt None: A alone)."""
    return [dict(n_model=it['n_p'] * it['n_t'], n_model_mod32=it['n_p'] * it['n_t'] % 32, n_masked=k,
                 n_pairs=N_METAL_PAIRS[it['kind']][0], n_main=N_METAL_PAIRS[it['kind']][1], n_metal_metal=N_METAL_PAIRS[it['kind']][2],
                 kron=(it['n_p'], None if it['rp_only'] else it['n_t'])) for it, k in zip(items, n_masked)]


def _metal_case(items, n_masked):
    return items, _metal_facts(items, n_masked)


# name -> (items, claimed facts); n_masked is a literal claim (check_metal_facts), the rest follows from the grid
METAL_CASES = {
    # less than one 256-thread block, n % 32 = 31; (n_rp, n_rt) % 5 = (2, 4)
    'm63': _metal_case([_metal_item('auto', 7, 9)], [59]),
    # rt tail empty, rp tail 4
    'm90': _metal_case([_metal_item('auto', 9, 10)], [86]),
    # the copy path of a missing rt factor at a ragged size (3); one exact row of 64
    'm64_rp': _metal_case([_metal_item('auto', 8, 8, rp_only=True)], [60]),
    # rp tail empty, rt tail 3; no r cut: every bin fitted
    'm65': _metal_case([_metal_item('auto', 5, 13, r_min=0.)], [65]),
    # (2, 2): the one grid with n_rt % 5 = 2
    'm84': _metal_case([_metal_item('auto', 7, 12)], [80]),
    # five 256-thread blocks + 16; (1, 1)
    'm1296': _metal_case([_metal_item('auto', 36, 36)], [1256]),
    # a cross-correlation: catalogue weights, rp symmetric about 0, 4 pairs; (0, 3)
    'mx1320': _metal_case([_metal_item('cross', 40, 33, z_scatter=0.02)], [1312]),
    # two items: the second item's metals start at metal_base = 15; a one-block item beside a six-block item in one launch
    'mj': _metal_case([_metal_item('auto', 7, 9), _metal_item('cross', 40, 33, z_scatter=0.02)], [59, 1312]),
}
# Problem-level variants of m63 (tests/test_metal_shapes_gpu.py), compared with the CPU oracle:
#   m63_mixed  two of the main x metal pairs lose their matrix: plain, groupable pairs next to matrix pairs in one item
#   m63_fast   fast_metals = True, chi2 at the fiducial point first: static vectors, shared pipelines, the static groups
METAL_VARIANTS = {'m63_mixed': 'm63', 'm63_fast': 'm63'}
MIXED_PLAIN_PAIRS = (1, 3)          # the pairs of m63_mixed without a matrix (indices into item.metals; both main x metal)


def check_metal_claims():
    """n_rp mod 5 and n_rt mod 5 each take every value 0...4 over the cases (a case without rt factor counts for n_rp only);
    every Kronecker set passes the LDS test of vmx_item_set_metal_kron; a grid below one 256-thread block, one with
    n % 32 != 0, one above five blocks, and a second item behind a first one with metals."""
    rp, rt, sizes = set(), set(), []
    for name, (items, facts) in METAL_CASES.items():
        assert len(items) == len(facts), name
        for item, fact in zip(items, facts):
            n_rp, n_rt = fact['kron']
            assert n_rp == item['n_p'] and fact['n_model'] == item['n_p'] * item['n_t'] and fact['n_model_mod32'] == fact['n_model'] % 32
            rp.add(n_rp % 5)
            if n_rt is not None:
                assert n_rt == item['n_t']
                rt.add(n_rt % 5)
            n = fact['n_model']
            assert (2 * n + max(n_rp * n_rp, item['n_t'] * item['n_t'])) * 8 <= KRON_LDS_BYTES, name
            assert fact['n_pairs'] == fact['n_main'] + fact['n_metal_metal'] <= 64      # (xi_sum_plan's metal mask)
            sizes.append(n)
    assert rp == {0, 1, 2, 3, 4}, sorted(rp)
    assert rt == {0, 1, 2, 3, 4}, sorted(rt)
    assert min(sizes) < 256 and max(sizes) > 5 * 256 and any(n % 32 for n in sizes) and any(n % 32 == 0 for n in sizes)
    assert any(f['kron'][1] is None and f['kron'][0] % 5 for _, facts in METAL_CASES.values() for f in facts)
    assert [f['n_pairs'] for f in METAL_CASES['mj'][1]] == [15, 4]
    assert set(METAL_VARIANTS.values()) <= set(METAL_CASES)
    assert all(i < N_METAL_PAIRS['auto'][1] for i in MIXED_PLAIN_PAIRS)


def metal_item_ini(text, item, directory, tag):
    """An item's ini text for `new_metals`: the data file of the item (with the picca cosmology in its header), the
    stacked-delta file and the object catalogue written under ``directory``, the [metals] section kept as it is (its file
    is not read then) and the [metal-matrix] section of vega_amd.synthetic appended."""
    from vega_amd import synthetic
    directory = Path(directory)
    stack = synthetic.write_stacked_deltas(directory / 'stack.fits')
    cat = synthetic.write_object_catalog(directory / 'cat.fits')
    lines = write_item_files(directory, item, tag)
    lines += f'\nweights-tracer1 = {stack}\nweights-tracer2 = {cat if item["kind"] == "cross" else stack}'
    text = adapt_item_ini(text, item, lines)
    assert text.count('[model]') == 1
    text = text.replace('[model]', '[model]\nnew_metals = True' + ('\nrp_only_metal_mats = True' if item['rp_only'] else ''))
    return text.rstrip('\n') + '\n\n' + synthetic.METAL_MATRIX_SECTION


def write_metal_case(tmp_path, case, golden):
    """write_case for METAL_CASES, starting from tests/golden/configs/auto_metals and configs/joint_metals."""
    tmp_path, golden = Path(tmp_path), Path(golden)
    items, _ = METAL_CASES[case]
    cfg = tmp_path / 'configs' / case
    cfg.mkdir(parents=True, exist_ok=True)
    single_auto = len(items) == 1 and items[0]['kind'] == 'auto'
    main = (golden / 'configs' / ('auto_metals' if single_auto else 'joint_metals') / 'main.ini').read_text()
    names = []
    for i, item in enumerate(items):
        config, name = METAL_ITEM_FILES[item['kind']]
        text = (golden / 'configs' / config / f'{name}.ini').read_text()
        (cfg / f'{name}.ini').write_text(metal_item_ini(text, item, tmp_path, f'{case}_{i}'))
        names.append(name)
    main = re.sub(r'ini files = .*', 'ini files = ' + ' '.join(f'configs/{case}/{n}.ini' for n in names), main)
    (cfg / 'main.ini').write_text(main)
    return f'configs/{case}/main.ini'


def check_metal_facts(case, problem):
    """The built Problem of a metal case against its claims."""
    items, facts = METAL_CASES[case]
    assert len(problem.items) == len(items)
    for item, fact, got in zip(items, facts, problem.items.values()):
        n_model, n_masked = got.model_grid.size, int(got.model_mask.sum())
        assert (n_model, n_model % 32, n_masked) == (fact['n_model'], fact['n_model_mod32'], fact['n_masked']), (case, n_model, n_masked)
        assert got.dist_grid.size == n_model == got.data_size + (n_model - n_masked) and not got.broadband
        assert got.distortion.shape == (n_model, n_model) and got.metal_opts['no_metal_decomp'] and not got.metal_opts['fast_metals']
        main = (got.tracer1.name, got.tracer2.name)
        with_main = [p.cross_with_main for p in got.metals]
        assert with_main == [p.names[0] in main or p.names[1] in main for p in got.metals]
        assert (len(got.metals), sum(with_main), len(got.metals) - sum(with_main)) == (fact['n_pairs'], fact['n_main'], fact['n_metal_metal']), \
            (case, len(got.metals), sum(with_main))
        n_rp, n_rt = fact['kron']
        for pair in got.metals:
            a, b = pair.kron
            assert a.shape == (n_rp, n_rp) and (b is None if n_rt is None else b.shape == (n_rt, n_rt)), (case, pair.names)
            assert pair.matrix.shape == (n_model, n_model) and pair.pipeline.r.size == n_model
        assert (got.model_grid.n_rp, got.model_grid.n_rt) == (item['n_p'], item['n_t'])


def metal_variant(problem, variant):
    """A Problem-level variant of a built metal case (a copy: the case's own Problem stays as it is)."""
    import copy
    prob = copy.copy(problem)
    prob.items = {}
    for name, item in problem.items.items():
        t = copy.copy(item)
        t.__dict__.pop('_oracle_xi_metal_metal', None)
        if variant == 'm63_mixed':
            t.metals = list(item.metals)
            for i in MIXED_PLAIN_PAIRS:
                pair = copy.copy(item.metals[i])
                assert pair.cross_with_main and pair.matrix is not None
                pair.matrix = None
                pair.kron = None
                t.metals[i] = pair
        elif variant == 'm63_fast':
            t.metal_opts = dict(item.metal_opts, fast_metals=True, fast_metal_bias=True)
        else:
            raise KeyError(variant)
        prob.items[name] = t
    return prob
