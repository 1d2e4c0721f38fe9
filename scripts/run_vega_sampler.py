#!/usr/bin/env python
"""Sample the posterior of a main config on one GPU: the reference's ``bin/run_vega_mpi.py`` for one process with
``[control] run_sampler = True`` and ``sampler = Ensemble`` (settings in ``[Ensemble]``: path, name, walkers, steps, seed, a,
thin, init, init_scale, driver) or ``sampler = Nested`` (``[Nested]``: path, name, num_live, num_repeats, precision, seed, threads,
driver, max_iterations) or ``sampler = SMC`` (``[SMC]``: path, name, particles, ess, sweeps, seed, driver, max_stages).  Writes
``<path>/<name>.txt`` and ``<path>/<name>.paramnames`` (getdist's plain-text chain); a nested or SMC run also
``<path>/<name>.stats`` with the evidence.  ``derived = True`` in the sampler's section appends the marginalisation
coefficients as derived parameters (``<corr>_marg_<i>``) to both files.

    python scripts/run_vega_sampler.py main.ini
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))


def main():
    pars = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                   description='Run the ensemble, nested or SMC sampler of vega_amd on one GPU.')
    pars.add_argument('config', type=str, help='Main config file')
    pars.add_argument('--search-dir', action='append', default=[], help='extra directories to look for input files in')
    pars.add_argument('--max-batch', type=int, default=256, help="the engine's batch size (walkers per chain launch)")
    args = pars.parse_args()
    from vega_amd import run_vega_sampler
    sampler = run_vega_sampler(args.config, search_dirs=args.search_dir, max_batch=args.max_batch)
    if hasattr(sampler, 'log_evidence') and hasattr(sampler, 'particles'):
        log_z, err = sampler.log_evidence()
        print(f'log(Z) = {log_z:.4f} +- {err:.4f}, {sampler.stage} stages, {sampler.stats["rows"]} likelihood evaluations in '
              f'{sampler.stats["seconds"]:.2f} s ({sampler.driver} driver)')
        return
    if hasattr(sampler, 'log_evidence'):
        log_z, err = sampler.log_evidence()
        print(f'log(Z) = {log_z:.4f} +- {err:.4f}, H = {sampler.information():.3f}, {sampler.iteration} iterations, '
              f'{sampler.stats["rows"]} likelihood evaluations in {sampler.stats["seconds"]:.2f} s ({sampler.driver} driver)')
        return
    print(f'acceptance fraction {sampler.acceptance_fraction.mean():.3f}, {sampler.stats["proposals"]} proposals in '
          f'{sampler.stats["seconds"]:.2f} s ({sampler.driver} driver)')


if __name__ == '__main__':
    main()
