#!/usr/bin/env python
"""What ``n_total`` and ``recycle`` cost the SMC sampler's device driver (vega_amd/smc.py), on the workload and by the protocol
of scripts/gpu_smc_rate.py: the synthetic joint problem with 6 sampled parameters, a warm-up, timed windows of at least
``--min-seconds``, fresh seeds.  Per N one JSON line with

  off            moves / s of runs of ``--stages`` stages with neither option: the figure of gpu_smc_rate.py --device-only, to be
                 held against the same script in a tree of the parent commit, the two alternating in one session
  n_total = 8 N  whole runs: the ladder in one call (as many stages as the plain run of that seed took: the ladder does not see the
                 rounds), then the 7 posterior rounds in another; moves / s, host waits and acceptance of each part
  recycle        whole runs with and without ``recycle`` under the same seeds, alternating: the seconds the kept positions cost
                 (the stage head's copy and the copy back of rec_u) as a share of the call

Not a test.

    python scripts/gpu_smc_keep_rate.py --particles 512 1024
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / 'tests'):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

SAMPLED = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'bias_hcd']
KEYS = ('rows', 'seconds', 'accepted', 'host_waits', 'stages')


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--particles', type=int, nargs='+', default=[512, 1024])
    pars.add_argument('--stages', type=int, default=6, help='stages per run of the part with the options off')
    pars.add_argument('--min-seconds', type=float, default=1.0, help='every timed window holds at least so much')
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--max-stages', type=int, default=60, help='a ladder longer than this is not waited for')
    args = pars.parse_args()
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import SMCSampler, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    for N in args.particles:
        kw = dict(particles=N, sample_params=sp)
        SMCSampler(vega, seed=1, **kw).run(stages=1)                                   # (warm-up: lanes, tables, code)
        SMCSampler(vega, seed=1, n_total=2 * N, recycle=True, max_stages=1, **kw).run()
        out = {'particles': N, 'max_batch': args.max_batch, 'sampled': len(SAMPLED)}
        # ---- off
        rows, sec, runs = 0, 0.0, 0
        while sec < args.min_seconds:
            s = SMCSampler(vega, seed=2 + runs, **kw).run(stages=args.stages)
            rows, sec, runs = rows + s.stats['rows'], sec + s.stats['seconds'], runs + 1
        out['off'] = {'moves_per_s': rows / sec, 'seconds': sec, 'runs': runs, 'sweeps': s.sweeps, 'lanes': s.stats['lanes']}
        # ---- n_total = 8 N, and recycle against plain under the same seeds
        ladder, rounds = dict.fromkeys(KEYS, 0), dict.fromkeys(KEYS, 0)
        plain_s, kept_s, runs = 0.0, 0.0, 0
        while rounds['seconds'] < args.min_seconds or plain_s < args.min_seconds:
            seed = 100 + runs
            plain = SMCSampler(vega, seed=seed, max_stages=args.max_stages, **kw).run()
            if not plain.finished:
                raise SystemExit(f'N = {N}, seed {seed}: the ladder has more than {args.max_stages} stages')
            kept = SMCSampler(vega, seed=seed, recycle=True, **kw).run()
            assert kept.stage == plain.stage and kept.stats['rows'] == plain.stats['rows']
            plain_s, kept_s = plain_s + plain.stats['seconds'], kept_s + kept.stats['seconds']
            top = SMCSampler(vega, seed=seed, n_total=8 * N, **kw).run(stages=plain.stage)
            assert top.beta == 1.0 and top.topups_left == 7 and len(top.record) == plain.stage
            for key in KEYS:
                ladder[key] += top.stats[key]
            before = {key: top.stats[key] for key in KEYS}
            top.run()
            assert top.finished and len(top.posterior_rounds) == 7
            for key in KEYS:
                rounds[key] += top.stats[key] - before[key]
            runs += 1
        for name, part in (('ladder', ladder), ('posterior_rounds', rounds)):
            starts = runs * N if name == 'ladder' else 0
            out[name] = {'moves_per_s': part['rows'] / part['seconds'], 'seconds': part['seconds'], 'stages': part['stages'],
                         'host_waits': part['host_waits'], 'acceptance': part['accepted'] / (part['rows'] - starts)}
        out['rounds_over_ladder'] = out['posterior_rounds']['moves_per_s'] / out['ladder']['moves_per_s']
        out['recycle'] = {'seconds_plain': plain_s, 'seconds_kept': kept_s, 'runs': runs,
                          'share_of_the_call': (kept_s - plain_s) / kept_s, 'n_eff_over_N': kept.n_eff() / N,
                          'kept_bytes_last_run': (kept.stage + 1) * N * len(SAMPLED) * 8}
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
