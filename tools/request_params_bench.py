"""Cost of per-request sampling parameters against the scalar call: d24 bf16 autoregressive_infer_cfg (incl. both decodes, the bench's
sampling settings cfg 4, top_k 900, top_p 0.96) eager at B = 512 and as one HIP graph at B = 8.  Per-request mode is handed UNIFORM
parameters (the same values in every row), so both modes do the same work on the same logits; one model in one process, the two modes
interleaved call by call so that clock and thermal drift fall on both alike.  Reports images/s of both, the spread of the scalar
repeats, and the sampler's kernel time per generation in both modes (HIP events around every sampling call of one extra eager generation).

Acceptance: per-request mode lies within the larger of 1 % and the spread of the scalar mode's own repeats.

    python tools/request_params_bench.py --out profiles/request_params_d24.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG, TOP_K, TOP_P = 4.0, 900, 0.96


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


def sampler_kernel_ms(fn):
    """kernel time of the sampling calls of one eager generation: HIP events around ops.cfg_sample / ops.cfg_sample_rows"""
    import torch
    from controlvar_amd import ops
    events = []
    saved = {name: getattr(ops, name) for name in ('cfg_sample', 'cfg_sample_rows')}

    def wrap(f):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(*a, **k)
            e1.record()
            events.append((e0, e1))
            return r
        return g
    try:
        for name, f in saved.items():
            setattr(ops, name, wrap(f))
        fn()
        torch.cuda.synchronize()
    finally:
        for name, f in saved.items():
            setattr(ops, name, f)
    return round(sum(e0.elapsed_time(e1) for e0, e1 in events), 3), len(events)


def compare(B, calls, reps, warmup):
    """calls: {'scalar': fn(i), 'per_request': fn(i)} -> medians, the scalar spread and the verdict"""
    times = {m: [] for m in calls}
    for i in range(warmup):
        for m in calls:
            timed(lambda: calls[m](i))
    for i in range(reps):
        order = ('scalar', 'per_request') if i % 2 == 0 else ('per_request', 'scalar')
        for m in order:
            times[m].append(timed(lambda: calls[m](100 + i)))
    med = {m: statistics.median(v) for m, v in times.items()}
    res = {m: {'ms_median': round(med[m] * 1e3, 3), 'ms_all': [round(t * 1e3, 3) for t in times[m]], 'images_per_s': round(B / med[m], 2)} for m in calls}
    spread = (max(times['scalar']) - min(times['scalar'])) / med['scalar']
    ratio = med['per_request'] / med['scalar']
    bound = max(0.01, spread)
    res.update(scalar_spread=round(spread, 5), per_request_over_scalar=round(ratio, 5), bound=round(bound, 5), within_bound=bool(ratio - 1.0 <= bound))
    return res


def run(a):
    import torch
    from controlvar_amd import models
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    out = {'config': f'd{a.depth} ControlVAR autoregressive_infer_cfg 256^2 incl. both decodes, bf16, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; scalar call '
                     f'and per-request mode with uniform parameters interleaved call by call on one model, median of {a.reps} calls each; the host table '
                     'build and its one host-to-device copy are inside the per-request time',
           'acceptance': 'per_request_over_scalar - 1 <= max(0.01, scalar_spread), scalar_spread = (max - min) / median of the scalar repeats',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    def uniform(B):
        return dict(cfg=[CFG] * B, top_k=[TOP_K] * B, top_p=[TOP_P] * B)

    # ---- eager, the headline batch
    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    calls = {'scalar': lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=i, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types),
             'per_request': lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=[i] * B, cond_type=types, **uniform(B))}
    res = compare(B, calls, a.reps, a.warmup)
    for m in calls:
        res[m]['sampler_kernel_ms_per_generation'], res[m]['sampler_calls'] = sampler_kernel_ms(lambda: calls[m](7))
    out[f'eager_B{B}'] = res
    print(f'[request_params] eager B={B}: ' + json.dumps(res), flush=True)

    # ---- captured, B = 8
    B = a.graph_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    eager = {'scalar': lambda: var.autoregressive_infer_cfg(B, labels, g_seed=7, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types),
             'per_request': lambda: var.autoregressive_infer_cfg(B, labels, g_seed=[7] * B, cond_type=types, **uniform(B))}
    kernel = {m: sampler_kernel_ms(f) for m, f in eager.items()}
    scalar = var.graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P)
    rows = var.graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P, per_request=True)
    calls = {'scalar': lambda i: scalar(labels, types, g_seed=i), 'per_request': lambda i: rows(labels, types, g_seed=[i] * B)}
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    for m in calls:
        res[m]['sampler_kernel_ms_per_generation'], res[m]['sampler_calls'] = kernel[m]
    res['sampler_kernel_note'] = f'measured on the eager B = {B} call of the same mode (events cannot sit inside the replayed graph)'
    out[f'graph_B{B}'] = res
    print(f'[request_params] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=512)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=9, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 3 or a.graph_reps < 3:
        ap.error('at least three repeats per mode')
    out = run(a)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
