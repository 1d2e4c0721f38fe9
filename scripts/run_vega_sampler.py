#!/usr/bin/env python
"""Sample the posterior of a main config, one process per GPU: the reference's ``bin/run_vega_mpi.py`` with
``[control] run_sampler = True`` and ``sampler = Ensemble`` (settings in ``[Ensemble]``: path, name, walkers, steps, seed, a,
thin, init, init_scale, driver) or ``sampler = Nested`` (``[Nested]``: path, name, num_live, num_repeats, precision, seed, threads,
driver, max_iterations, do_clustering, cluster_posteriors, boost_posterior) or ``sampler = SMC`` (``[SMC]``: path, name, particles, ess, sweeps, seed, driver, max_stages).  Writes
``<path>/<name>.txt`` and ``<path>/<name>.paramnames`` (getdist's plain-text chain); a nested or SMC run also
``<path>/<name>.stats`` with the evidence.  ``derived = True`` in the sampler's section appends the marginalisation
coefficients as derived parameters (``<corr>_marg_<i>``) to both files.

    python scripts/run_vega_sampler.py main.ini

``replicas = R`` in the sampler's section runs R independent copies (the same seed, Philox stream r) and merges them
(vega_amd/replicas.py): nested runs into one run with the summed live count, SMC evidences into their mean, ensembles into
``<name>_1.txt ... <name>_R.txt`` with R-hat in ``<name>.stats``.  ``together = True`` beside it (``[Ensemble]``, ``[SMC]``,
``[Nested]``) advances a rank's replicas as one set in one device run; ``mocks = M`` in the sampler's section (Monte-Carlo mode)
samples every one of M mocks in one run and writes ``<name>_mock<m>.*`` with ``mock_posteriors.fits``.  The ranks share the replicas out in contiguous blocks and run
theirs one after the other; every replica leaves ``<name>.replica<r>.npz``; rank 0 merges.  Under torchrun (gloo carries two
barriers and one gather of counts; there is no data-path collective):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29556 \
        scripts/run_vega_sampler.py main.ini

or let the script start the ranks itself - fresh child processes, rank r on GPU r % (number of GPUs); the parent never
touches a GPU, every child runs under ``--timeout``, and the first child that fails ends the run with its status:

    python scripts/run_vega_sampler.py main.ini --ranks 8
"""
import argparse
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

MAX_RANKS = 16


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _stop(procs):
    for p in procs:
        if p.poll() is None:
            p.terminate()
    for p in procs:
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def launch(argv, ranks, timeout):
    """Start ``ranks`` fresh processes of this script (``argv``: its arguments without ``--ranks``) with ``RANK`` / ``WORLD_SIZE``
    / ``LOCAL_RANK`` set and wait for them.  Returns 0 when all ended well; the status of the first child that failed (the others
    are ended, nothing is started again); 124 when ``timeout`` seconds passed."""
    port = _free_port()
    procs = []
    for r in range(ranks):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(ranks), LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve())] + list(argv), env=env))
    deadline = time.monotonic() + timeout
    try:
        while True:
            codes = [p.poll() for p in procs]
            failed = [c for c in codes if c not in (None, 0)]
            if failed:
                print(f'rank {codes.index(failed[0])} ended with status {failed[0]}: ending the run', file=sys.stderr)
                return failed[0] if failed[0] > 0 else 1
            if all(c == 0 for c in codes):
                return 0
            if time.monotonic() > deadline:
                print(f'the ranks did not finish within {timeout} s: ending the run', file=sys.stderr)
                return 124
            time.sleep(0.2)
    finally:
        _stop(procs)


def report(out):
    """One line about what :func:`vega_amd.run_vega_sampler` returned."""
    if out is None:
        return
    if hasattr(out, 'summary'):
        print(out.summary())
        return
    sampler = out
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


def main(argv=None):
    pars = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                   description='Run the ensemble, nested or SMC sampler of vega_amd, one process per GPU.')
    pars.add_argument('config', type=str, help='Main config file')
    pars.add_argument('--search-dir', action='append', default=[], help='extra directories to look for input files in')
    pars.add_argument('--max-batch', type=int, default=256, help="the engine's batch size (walkers per chain launch)")
    pars.add_argument('--ranks', type=int, default=None,
                      help=f'start this many rank processes (at most {MAX_RANKS}) instead of running under torchrun')
    pars.add_argument('--timeout', type=float, default=86400.0, help='seconds the rank processes of --ranks may take')
    args = pars.parse_args(argv)
    if args.ranks is not None:
        if not 1 <= args.ranks <= MAX_RANKS:
            pars.error(f'--ranks: 1 .. {MAX_RANKS}')
        if not args.timeout > 0:
            pars.error('--timeout: a positive number of seconds')
        child = [args.config, '--max-batch', str(args.max_batch)]
        for d in args.search_dir:
            child += ['--search-dir', d]
        return launch(child, args.ranks, args.timeout)
    from vega_amd import run_vega_sampler
    rank = int(os.environ.get('RANK', '0'))
    try:
        out = run_vega_sampler(args.config, search_dirs=args.search_dir, max_batch=args.max_batch)
        if rank == 0:
            report(out)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
