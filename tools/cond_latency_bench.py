#!/usr/bin/env python3
"""Small-batch latency of conditional generation (control in, image out; image in, control out): the eager launch sequence a user writes -
`vae.img_to_idxBl(pixels)` then `conditional_infer_cfg(c_mask= / c_img=)` - against one replay of `graphed_conditional_generator(source='pixels')`,
which holds tokeniser + generation + decode.  d24 ControlVAR + ch160 VQVAE, bf16, cfg (4, 4, 4), top_k 900 / top_p 0.96, synthetic control
pixels (controlvar_amd.synth).  For every B and both `given` values the three paths (eager, replay decode='both', replay decode='generated')
run interleaved call by call in one process, each call bracketed by a device synchronise; median and spread of --reps calls after --warmup.

    python tools/cond_latency_bench.py --out profiles/cond_graph_d24.json

The parent process never opens the GPU: every batch size is one child process under its own `timeout -k 10`, and the first child that fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATHS = ('eager', 'graph_both', 'graph_generated')


def lib_digest():
    try:
        return open(os.path.join(ROOT, 'controlvar_amd', 'csrc', 'build', 'digest.txt')).read().strip()[:16]
    except OSError:
        return None


def stats(v):
    ms = sorted(x * 1e3 for x in v)
    return {'ms_median': round(statistics.median(ms), 2), 'ms_min': round(ms[0], 2), 'ms_max': round(ms[-1], 2), 'ms_stdev': round(statistics.stdev(ms), 3),
            'calls': len(ms)}


def cell(a, B):
    """one batch size, both directions: runs in a child process"""
    import torch
    from controlvar_amd import models, ops
    from controlvar_amd.synth import synth_images
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(ch=160, compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    sampling = dict(cfg=(4.0, 4.0, 4.0), top_k=900, top_p=0.96)
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    pix = synth_images(B, 16 * var.patch_nums[-1], seed=7).to(dev)
    out = {'device': torch.cuda.get_device_name(dev)}
    for given in ('control', 'image'):
        teach = 'c_mask' if given == 'control' else 'c_img'

        def eager(i):
            return var.conditional_infer_cfg(B, labels, g_seed=i, cond_type=types, **sampling, **{teach: vae.img_to_idxBl(pix)})
        eager(0)
        torch.cuda.synchronize()
        # library calls of one eager generation (tokeniser + generation + decode): each is at least one kernel launch, and the graph holds the same ones
        calls, check = [0], ops.check

        def counting(*args, **kw):
            calls[0] += 1
            return check(*args, **kw)
        ops.check = counting
        try:
            eager(0)
        finally:
            ops.check = check
        torch.cuda.synchronize()
        runs = {'eager': eager}
        for decode in ('both', 'generated'):
            run = var.graphed_conditional_generator(B, given=given, source='pixels', decode=decode, **sampling)
            runs['graph_' + decode] = (lambda i, run=run: run(labels, types, pix, g_seed=i))
        times = {p: [] for p in PATHS}

        def call(p, i):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[p](i)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        for i in range(a.warmup):
            for p in PATHS:
                call(p, i)
        for i in range(a.reps):
            for p in PATHS[i % 3:] + PATHS[:i % 3]:          # rotate the order: clock and thermal drift fall on all three alike
                times[p].append(call(p, 100 + i))
        res = {p: stats(v) for p, v in times.items()}
        res['library_calls_per_eager_generation'] = calls[0]
        res['eager_over_graph_both'] = round(res['eager']['ms_median'] / res['graph_both']['ms_median'], 3)
        res['eager_over_graph_generated'] = round(res['eager']['ms_median'] / res['graph_generated']['ms_median'], 3)
        out[f'given_{given}'] = res
        print(f'[cond_latency] B={B} given={given}: ' + json.dumps(res), flush=True)
        del runs, run
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step-timeout', type=int, default=420, help='seconds per batch size (one child process each)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--cell', type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--cell-out', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error('--reps: at least 20 timed calls per cell')
    if a.cell is not None:
        res = cell(a, a.cell)
        with open(a.cell_out, 'w') as f:
            json.dump(res, f)
        return
    out = {'config': f'd{a.depth} ControlVAR + ch160 VQVAE, bf16, conditional generation 256^2 from synthetic control pixels, cfg (4, 4, 4), top_k 900, top_p 0.96, one GPU; '
                     f'eager = vae.img_to_idxBl(pixels) + conditional_infer_cfg, graph = one replay of graphed_conditional_generator(source=\'pixels\'); the three '
                     f'paths interleaved call by call in one process, every call bracketed by a device synchronise, {a.warmup} warm-up + {a.reps} timed calls each',
           'lib_digest': lib_digest()}
    with tempfile.TemporaryDirectory() as tmp:
        for B in a.batch:
            part = os.path.join(tmp, f'B{B}.json')
            cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--depth', str(a.depth), '--reps', str(a.reps),
                   '--warmup', str(a.warmup), '--cell', str(B), '--cell-out', part]
            rc = subprocess.call(cmd)
            if rc != 0:                                         # a failed step ends the run: nothing more is started on the GPU
                sys.exit(f'[cond_latency] B={B} ended with status {rc}; stopping')
            res = json.load(open(part))
            out.setdefault('device', res.pop('device'))
            out[f'B{B}'] = res
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
