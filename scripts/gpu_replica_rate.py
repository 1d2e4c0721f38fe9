#!/usr/bin/env python
"""Aggregate likelihood rows / s of 1, 2 or 4 rank processes that share ONE GPU, each running a replica of a device sampler
(vega_amd/replicas.py: replica r = Philox stream r) on the synthetic joint problem of scripts/gpu_nested_rate.py with 6 sampled
parameters.  A sampler step is a dependent chain of short batches with one decision kernel between them; a single process
leaves gaps between them.  This measures whether a second and a fourth process fill those gaps.  Not a test; no threshold.

One call measures one process count: the parent starts ``--processes N`` fresh worker processes (it makes no GPU call itself),
every worker builds its engine, warms up, and then meets the others at a gloo barrier before each timed run, so that the timed
windows overlap.  Prints one JSON line: per sampler the summed rows over the slowest worker's seconds, and each worker's own
figures.  Run the counts as separate, time-limited steps that stop at the first failure:

    timeout -k 10 400 python scripts/gpu_replica_rate.py --processes 1 && \
    timeout -k 10 400 python scripts/gpu_replica_rate.py --processes 2 && \
    timeout -k 10 400 python scripts/gpu_replica_rate.py --processes 4

What N GPUs gain in wall-clock time cannot be read off a one-GPU box: replicas on separate GPUs share nothing but two barriers.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / 'tests'):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

SAMPLED = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'bias_hcd']
MAX_PROCESSES = 16


def worker(args):
    import torch
    import torch.distributed as dist
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, NestedSampler, SMCSampler, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)

    def together():
        if world > 1:
            dist.barrier()

    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    out = {'rank': rank}
    # warm-up of all three (lanes, tables, code) before anything is timed
    NestedSampler(vega, num_live=args.num_live, seed=1, sample_params=sp).run(iterations=1)
    SMCSampler(vega, particles=args.particles, seed=1, sample_params=sp).run(stages=1)
    EnsembleSampler(vega, args.walkers, seed=1, sample_params=sp).run(2, start='prior')
    runs = {'nested': lambda: NestedSampler(vega, num_live=args.num_live, seed=2, stream=rank, sample_params=sp)
            .run(iterations=args.iterations),
            'smc': lambda: SMCSampler(vega, particles=args.particles, seed=2, stream=rank, sample_params=sp).run(stages=args.stages),
            'ensemble': lambda: EnsembleSampler(vega, args.walkers, seed=2, stream=rank, sample_params=sp)
            .run(args.steps, start='prior')}
    for name, run in runs.items():
        together()
        t0 = time.perf_counter()
        s = run()
        dt = time.perf_counter() - t0
        rows = s.stats['rows'] if name != 'ensemble' else s.stats['proposals']
        out[name] = {'rows': int(rows), 'seconds': dt, 'rows_per_s': rows / dt}
    together()
    vega.close()
    if world > 1:
        dist.destroy_process_group()
    print('RESULT ' + json.dumps(out), flush=True)


def parent(args):
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    argv = [sys.executable, str(Path(__file__).resolve()), '--worker'] + [
        f'--{k.replace("_", "-")}={getattr(args, k)}' for k in ('num_live', 'iterations', 'particles', 'stages', 'walkers', 'steps',
                                                                 'max_batch')]
    procs = []
    for r in range(args.processes):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.processes), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen(argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    deadline = time.monotonic() + args.timeout
    status = 0
    while any(p.poll() is None for p in procs):             # the first failure ends the measurement; nothing is started again
        bad = [p.returncode for p in procs if p.poll() not in (None, 0)]
        if bad or time.monotonic() > deadline:
            status = bad[0] if bad else 124
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            break
        time.sleep(0.2)
    outputs = []
    for p in procs:
        try:
            outputs.append(p.communicate(timeout=15)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outputs.append(p.communicate()[0])
    status = status or next((p.returncode for p in procs if p.returncode), 0)
    if status:
        for r, text in enumerate(outputs):
            print(f'--- worker {r} (status {procs[r].returncode})\n{text[-3000:]}', file=sys.stderr)
        return status if status > 0 else 1
    results = [json.loads(line[7:]) for text in outputs for line in text.splitlines() if line.startswith('RESULT ')]
    out = {'processes': args.processes, 'max_batch': args.max_batch, 'sampled': len(SAMPLED),
           'settings': {'num_live': args.num_live, 'iterations': args.iterations, 'particles': args.particles, 'stages': args.stages,
                        'walkers': args.walkers, 'steps': args.steps}}
    for name in ('nested', 'smc', 'ensemble'):
        rows = sum(r[name]['rows'] for r in results)
        slowest = max(r[name]['seconds'] for r in results)
        out[name] = {'aggregate_rows_per_s': rows / slowest, 'rows': rows, 'slowest_seconds': slowest,
                     'per_process_rows_per_s': [r[name]['rows_per_s'] for r in sorted(results, key=lambda r: r['rank'])]}
    print(json.dumps(out), flush=True)
    return 0


def main():
    pars = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    pars.add_argument('--processes', type=int, default=1, help=f'worker processes sharing the GPU (at most {MAX_PROCESSES})')
    pars.add_argument('--timeout', type=float, default=360.0, help='seconds the workers may take')
    pars.add_argument('--num-live', type=int, default=512)
    pars.add_argument('--iterations', type=int, default=12)
    pars.add_argument('--particles', type=int, default=1024)
    pars.add_argument('--stages', type=int, default=4, help='SMC stages per run (24 sweeps each)')
    pars.add_argument('--walkers', type=int, default=512)
    pars.add_argument('--steps', type=int, default=60)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = pars.parse_args()
    if args.worker:
        return worker(args)
    if not 1 <= args.processes <= MAX_PROCESSES:
        pars.error(f'--processes: 1 .. {MAX_PROCESSES}')
    return parent(args)


if __name__ == '__main__':
    sys.exit(main())
