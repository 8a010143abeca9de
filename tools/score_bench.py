"""Cost of token log-probabilities: the per-request joint call without and with logprobs=True, d24 bf16 (incl. both decodes, the bench's
sampling settings cfg 4, top_k 900, top_p 0.96), eager at B = 512 and as one HIP graph at B = 8.  Both modes run on one model in one process,
interleaved call by call so that clock and thermal drift fall on both alike:

    per_request   autoregressive_infer_cfg in per-request mode (uniform parameters) - the baseline, whose code this feature does not touch
    logprobs      the same call with logprobs=True: one score launch per scale more, and (B, L) score buffers returned

Reports images/s of each, the ratio and the spread of the baseline's repeats.  The yardstick of the earlier features: the ratio should stay
within the larger of 1 % and that spread; the measured ratio is reported whether or not it meets that.

Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o score -- python tools/score_bench.py --trace
    python tools/score_bench.py --out profiles/score_d24.json --kernel-stats DIR/score_kernel_stats.csv

--trace runs the logprobs call alone a few times (eager, --trace-batch); --kernel-stats reads the resulting statistics and records the
per-generation time of the score kernel beside that of the sampler kernels.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG, TOP_K, TOP_P = 4.0, 900, 0.96
BASE, MODE = 'per_request', 'logprobs'
TRACE_CALLS = 3


def lib_digest():
    try:
        return open(os.path.join(ROOT, 'controlvar_amd', 'csrc', 'build', 'digest.txt')).read().strip()[:16]
    except OSError:
        return None


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def compare(B, calls, reps, warmup):
    """calls: {mode: fn(i)} -> medians, the baseline's spread and the ratio"""
    modes = list(calls)
    times = {m: [] for m in modes}
    for i in range(warmup):
        for m in modes:
            timed(lambda: calls[m](i))
    for i in range(reps):
        for m in modes[i % len(modes):] + modes[:i % len(modes)]:           # rotate the order: no mode always runs behind the other
            times[m].append(timed(lambda: calls[m](100 + i)))
    med = {m: statistics.median(v) for m, v in times.items()}
    res = {m: {'ms_median': round(med[m] * 1e3, 3), 'ms_all': [round(t * 1e3, 3) for t in times[m]], 'images_per_s': round(B / med[m], 2)} for m in modes}
    spread = (max(times[BASE]) - min(times[BASE])) / med[BASE]
    bound = max(0.01, spread)
    res.update(baseline_spread=round(spread, 5), bound=round(bound, 5), logprobs_over_per_request=round(med[MODE] / med[BASE], 5),
               logprobs_within_bound=bool(med[MODE] / med[BASE] - 1.0 <= bound))
    return res


def build(depth):
    import torch
    from controlvar_amd import models
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(compute_dtype=bf).to(dev)
    return dev, models.build_control_var(vae, depth=depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()


def uniform(B):
    return dict(cfg=[CFG] * B, top_k=[TOP_K] * B, top_p=[TOP_P] * B)


def trace(a):
    """the logprobs call alone, for a kernel trace: one warm-up and TRACE_CALLS calls (the statistics then hold 1 + TRACE_CALLS generations)"""
    import torch
    dev, var = build(a.depth)
    B = a.trace_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    for i in range(1 + TRACE_CALLS):
        var.autoregressive_infer_cfg(B, labels, g_seed=[i] * B, cond_type=types, logprobs=True, **uniform(B))
    torch.cuda.synchronize()
    print(f'[score_bench] traced {1 + TRACE_CALLS} generations at B = {B}')


def kernel_stats(path, generations):
    """per-generation kernel time (ms) of the score kernel and of the sampler kernels from a rocprofv3 kernel statistics file"""
    score = sampler = 0.0
    calls = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name']
            if 'cfg_score_rows_kernel' in name:
                score += float(row['TotalDurationNs'])
                calls['score'] = calls.get('score', 0) + int(row['Calls'])
            elif 'cfg_sample' in name or 'cfg_greedy' in name:
                sampler += float(row['TotalDurationNs'])
                calls['sampler'] = calls.get('sampler', 0) + int(row['Calls'])
    return {'generations': generations, 'launches': calls, 'score_kernel_ms_per_generation': round(score / generations / 1e6, 4),
            'sampler_kernels_ms_per_generation': round(sampler / generations / 1e6, 4),
            'score_over_sampler': round(score / sampler, 4) if sampler else None}


def run(a):
    import torch
    dev, var = build(a.depth)
    out = {'config': f'd{a.depth} ControlVAR 256^2 incl. both decodes, bf16, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; the per-request joint call '
                     '(uniform parameters) without and with logprobs=True, interleaved call by call on one model, median of the timed calls of each',
           'yardstick': 'logprobs_over_per_request - 1 <= max(0.01, baseline_spread), baseline_spread = (max - min) / median of the per_request repeats',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    # ---- eager, the headline batch
    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    calls = {BASE: lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=[i] * B, cond_type=types, **uniform(B)),
             MODE: lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=[i] * B, cond_type=types, logprobs=True, **uniform(B))}
    res = compare(B, calls, a.reps, a.warmup)
    out[f'eager_B{B}'] = res
    print(f'[score_bench] eager B={B}: ' + json.dumps(res), flush=True)

    # ---- captured, B = 8
    B = a.graph_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    rows = var.graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P, per_request=True)
    scored = var.graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P, per_request=True, logprobs=True)
    calls = {BASE: lambda i: rows(labels, types, g_seed=[i] * B), MODE: lambda i: scored(labels, types, g_seed=[i] * B)}
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    img, sc = scored(labels, types, g_seed=[0] * B)
    res['mean_logprob_per_token'] = round(float(sc.logprob.double().mean()), 4)
    res['mean_entropy_per_token'] = round(float(sc.entropy.double().mean()), 4)
    out[f'graph_B{B}'] = res
    print(f'[score_bench] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=512)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=9, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--trace', action='store_true', help='run the logprobs call alone a few times, for a kernel trace')
    ap.add_argument('--trace-batch', type=int, default=512)
    ap.add_argument('--kernel-stats', default=None, help='kernel statistics (csv) of a --trace run under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.trace:
        return trace(a)
    if a.reps < 3 or a.graph_reps < 3:
        ap.error('at least three repeats per mode')
    out = run(a)
    if a.kernel_stats:
        out[f'kernels_eager_B{a.trace_batch}'] = kernel_stats(a.kernel_stats, 1 + TRACE_CALLS)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
