"""Two batches in flight inside one engine (include/vegamx.h: vmx_set_lanes): the second lane borrows every static tensor
and owns its workspace and stream.  Per batch the arithmetic is one lane's: chi2 must be bit-for-bit what a single lane
gives, whatever is interleaved - and anything that changes what an evaluation computes must retire the clone."""
import numpy as np
import pytest

from conftest import load_problem, synth_joint_problem

pytestmark = pytest.mark.gpu

VARIED = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'sigma_velo_disp_lorentz_QSO', 'drp_QSO', 'bias_hcd', 'beta_hcd',
          'L0_hcd', 'bao_amp', 'bias_eta_SiII(1260)', 'bias_eta_CIV(eff)']


@pytest.mark.parametrize('tag,batch', [('joint_synth', 256), ('joint_metals', 96)])
def test_two_lanes_equal_one_lane_bitwise(tag, batch):
    import torch
    from vega_amd import VegaInterface, synthetic
    prob = synth_joint_problem() if tag == 'joint_synth' else load_problem(tag)
    vega = VegaInterface(None, problem=prob, max_batch=batch)
    eng = vega.engine
    eng.set_constant_nl_hint(True, gaussian=True)
    dev = torch.device('cuda', 0)
    pools = [torch.from_numpy(synthetic.walkers(eng.low.theta0, eng.names, batch, varied=VARIED, seed=100 + i)).to(dev)
             for i in range(6)]
    one = [torch.zeros(batch, dtype=torch.float64, device=dev) for _ in pools]
    for th, out in zip(pools, one):
        eng.eval_device(th.data_ptr(), batch, out.data_ptr())
    eng.sync()
    assert all(bool(torch.isfinite(o).all()) and bool((o < 1e99).all()) for o in one)
    eng.set_lanes(2)
    for rounds in range(3):
        two = [torch.zeros(batch, dtype=torch.float64, device=dev) for _ in pools]
        for th, out in zip(pools, two):
            eng.eval_device(th.data_ptr(), batch, out.data_ptr())
        eng.sync()
        for a, b in zip(one, two):
            assert torch.equal(a, b)
        # the host entry in between (it waits for the second lane and runs on the first)
        host = vega.chi2_batch(pools[1].cpu().numpy())
        np.testing.assert_array_equal(host, one[1].cpu().numpy())
    # the convenience entry (chunks alternate between the lanes)
    big = torch.cat(pools)
    got = vega.chi2_batch_device(big)
    assert torch.equal(got, torch.cat(one))
    # new data retire the clone: both lanes then see them
    item = next(iter(prob.items.values()))
    name = next(iter(prob.items))
    eng.set_data(name, 1.01 * item.masked_data_vec)
    two = [torch.zeros(batch, dtype=torch.float64, device=dev) for _ in pools]
    for th, out in zip(pools, two):
        eng.eval_device(th.data_ptr(), batch, out.data_ptr())
    eng.sync()
    eng.set_lanes(1)
    ref = [torch.zeros(batch, dtype=torch.float64, device=dev) for _ in pools]
    for th, out in zip(pools, ref):
        eng.eval_device(th.data_ptr(), batch, out.data_ptr())
    eng.sync()
    for a, b, c in zip(two, ref, one):
        assert torch.equal(a, b) and not torch.equal(a, c)
    vega.close()


@pytest.mark.parametrize('kind', ['ensemble', 'smc'])
def test_an_evaluation_of_a_main_lane_chunk_a_second_lane_chunk_and_a_ragged_tail(kind, monkeypatch):
    """The shared evaluate of the device drivers where its three chunk kinds meet after a rows-ready event was published:
    max_batch = 256, chunk = 64, two lanes, 160 rows per evaluation = 64 (main lane) + 64 (second lane) + 32 (below the 64-row
    floor of two lanes: it waits for the lane and runs on the main stream).  The two drivers that publish the event: the
    ensemble sampler (320 walkers, halves of 160, 3 steps) and SMC (160 particles, 3 sweeps, 1 stage)."""
    import test_ensemble_gpu as TE
    import test_smc_gpu as TS
    from vega_amd import EnsembleSampler, SMCSampler, VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        sp = TE._sample_params(vega, TE.AUTO_SAMPLED)
        if kind == 'ensemble':
            whole = EnsembleSampler(vega, 320, seed=7, sample_params=sp, chunk=0, lanes=2).run(3)
            seen = []       # (the sampler's own statistics do not carry the lanes: the engine's do)
            run = vega.engine.ensemble_run
            monkeypatch.setattr(vega.engine, 'ensemble_run', lambda *a, **k: seen.append(run(*a, **k)) or seen[-1])
            dev, py = TE._pair(vega, 320, 3, sp, chunk=64, lanes=2)
            TE._assert_same(dev, py)
            assert [st['lanes'] for _, _, st in seen] == [2]
            assert dev.stats['engine_calls'] == py.stats['engine_calls'] == 3 * (3 * 2)
            assert whole.stats['engine_calls'] == 3 * 2
            assert np.array_equal(dev.get_chain(), whole.get_chain()) and np.array_equal(dev.accepted, whole.accepted)
            np.testing.assert_allclose(dev.get_log_lik(), whole.get_log_lik(), rtol=1e-12, atol=0)
        else:
            kw = dict(particles=160, sweeps=3, seed=3)
            whole = SMCSampler(vega, sample_params=sp, chunk=0, lanes=2, **kw).run(stages=1)
            dev, py = TS._pair(vega, sp, 1, chunk=64, lanes=2, **kw)
            TS._assert_same(dev, py)
            assert dev.stage == 1 and dev.stats['lanes'] == 2
            assert dev.stats['engine_calls'] == py.stats['engine_calls'] == 3 * (1 + 3)
            assert whole.stats['engine_calls'] == 1 + 3
            assert np.array_equal(dev.u, whole.u) and dev.stage == whole.stage
            np.testing.assert_allclose(dev.lnl, whole.lnl, rtol=1e-12, atol=0)
    finally:
        vega.close()
