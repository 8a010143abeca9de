"""What gemm_precision='bf16x3' costs and buys: d24 ControlVAR 256^2 incl. both decodes, the bench's sampling settings (cfg 4, top_k 900, top_p 0.96), the
three precision modes interleaved call by call in one process so that clock and thermal drift fall on all alike:

    bf16     compute_dtype=bfloat16                       (throughput mode)
    bf16x3   compute_dtype=float32, gemm_precision='bf16x3'  (the fp32 model, linear layers as split-bf16 products on the bf16 tiles)
    fp32     compute_dtype=float32                        (parity mode: exact-f32 MFMA) - the baseline of the comparison

Eager at --eager-batch (default 64: the batch of bench.py's fp32 figure, and the largest power of two at which the K/V arenas of all three models - 51 GB
each for the two fp32-arena models, 26 GB for bf16, of the 802 MB per image an fp32 d24 arena takes - sit side by side in one process with the
activations of the last scale; B = 256 alone is 205 GB), and as one HIP graph at --graph-batch (8).  Reports per mode ms, images/s and the peak
allocation of a call, the spread of the fp32 baseline's repeats and the ratio fp32 / bf16x3.

The one condition: bf16x3 must beat fp32 by more than the larger of 1 % and the baseline's spread (`x3_beats_fp32`); the figure is reported either way.

A kernel-time breakdown of the mode comes from a run of its own (tracing slows the host; never combined with the timing above):

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/x3_bench.py --profile-only
    python tools/x3_bench.py --shares OUT/.../*_kernel_stats.csv          # GEMMs / attention / split3 + ln_modulate_split3 / decoder / other

    python tools/x3_bench.py --out profiles/x3_d24.json
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
MODES = ('bf16', 'bf16x3', 'fp32')
BASE = 'fp32'


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
    """calls: {mode: fn(i)} -> per-mode medians and peak allocation, the baseline's spread, the ratio and the verdict"""
    import torch
    modes = list(calls)
    times = {m: [] for m in modes}
    peak = {}
    for i in range(warmup):
        for m in modes:
            torch.cuda.reset_peak_memory_stats()
            timed(lambda: calls[m](i))
            peak[m] = torch.cuda.max_memory_allocated()           # (all three models resident: the peak of a call includes the other modes' weights and arenas)
    for i in range(reps):
        for m in modes[i % len(modes):] + modes[:i % len(modes)]:           # rotate the order: no mode always runs behind the same one
            times[m].append(timed(lambda: calls[m](100 + i)))
    med = {m: statistics.median(v) for m, v in times.items()}
    res = {m: {'ms_median': round(med[m] * 1e3, 3), 'ms_all': [round(t * 1e3, 3) for t in times[m]], 'images_per_s': round(B / med[m], 2),
               'peak_allocated_GB_all_models_resident': round(peak[m] / 1e9, 2)} for m in modes}
    spread = (max(times[BASE]) - min(times[BASE])) / med[BASE]
    bound = max(0.01, spread)
    gain = med[BASE] / med['bf16x3']
    res.update(baseline_spread=round(spread, 5), bound=round(bound, 5), fp32_over_bf16x3=round(gain, 4), bf16x3_over_bf16=round(med['bf16x3'] / med['bf16'], 4),
               x3_beats_fp32=bool(gain - 1.0 > bound))
    return res


def build(depth, dev, modes=MODES):
    import torch
    from controlvar_amd import models
    out = {}
    for mode in modes:
        dt = torch.bfloat16 if mode == 'bf16' else torch.float32
        vae = models.build_vae(compute_dtype=dt).to(dev)
        m = models.build_control_var(vae, depth=depth, mask_type='interleave_append', multi_cond=True, compute_dtype=dt,
                                     gemm_precision='bf16x3' if mode == 'bf16x3' else None).to(dev).eval()
        m._pack(); vae._pack()
        torch.cuda.synchronize()
        out[mode] = (m, torch.cuda.memory_allocated())
    return out


def run(a):
    import torch
    dev = torch.device('cuda:0')
    base_alloc = torch.cuda.memory_allocated()
    built = build(a.depth, dev)
    var = {k: v[0] for k, v in built.items()}
    after, weights = base_alloc, {}
    for mode in MODES:                                           # resident bytes each model added: parameters, packed copies, its VQVAE
        weights[mode] = round((built[mode][1] - after) / 1e9, 2)
        after = built[mode][1]
    out = {'config': f'd{a.depth} ControlVAR 256^2 incl. both decodes, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; autoregressive_infer_cfg of three models '
                     '(bf16 / fp32 + bf16x3 / fp32) interleaved call by call in one process, median of the timed calls of each',
           'acceptance': 'fp32_over_bf16x3 - 1 > max(0.01, baseline_spread), baseline_spread = (max - min) / median of the fp32 repeats',
           'resident_GB_added_per_model': weights, 'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    calls = {m: (lambda i, m=m: var[m].autoregressive_infer_cfg(B, labels, g_seed=i, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types)) for m in MODES}
    res = compare(B, calls, a.reps, a.warmup)
    out[f'eager_B{B}'] = res
    print(f'[x3_bench] eager B={B}: ' + json.dumps(res), flush=True)
    for m in MODES:
        var[m]._arena = None
    torch.cuda.empty_cache()

    B = a.graph_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    graphs = {m: var[m].graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P) for m in MODES}
    calls = {m: (lambda i, m=m: graphs[m](labels, types, g_seed=i)) for m in MODES}
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    out[f'graph_B{B}'] = res
    print(f'[x3_bench] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def profile_only(a):
    """the bf16x3 model alone, one warm-up and one generation at --eager-batch: the process rocprofv3 traces"""
    import torch
    dev = torch.device('cuda:0')
    m = build(a.depth, dev, modes=('bf16x3',))['bf16x3'][0]
    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    for i in range(2):
        m.autoregressive_infer_cfg(B, labels, g_seed=i, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types)
    torch.cuda.synchronize()
    print(f'[x3_bench] profile-only: two bf16x3 generations at B={B} done', flush=True)


# the VQVAE of this mode is the fp32 one: its convs and GEMMs are the <float, ...> instances of the tile kernel, the transformer's GEMMs the bf16 ones
GROUPS = (('split3_and_ln_modulate_split3', ('split3_kernel', 'bf16x3_t')),
          ('decoder_and_quantizer', ('cvar_gemm_kernel<float', 'conv3x3', 'gn_', 'softmax_rows', 'transpose_kernel', 'ms_', 'ms32', 'resample_sep', 'embed_rows',
                                     'nchw', 'nhwc', 'rowsum')),
          ('gemm', ('cvar_gemm', 'cvar_splitk')), ('attention', ('attn_', 'cos_qk_norm')), ('sampler', ('cfg_',)))


def shares(path):
    """kernel-time shares of a rocprofv3 --stats csv by kernel family (names matched in the order of GROUPS; the split-store adaLN carries bf16x3_t in its name)"""
    tot, by, names = 0.0, {}, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            ns = float(row.get('TotalDurationNs') or row.get('TotalDuration(ns)') or 0)
            grp = next((g for g, keys in GROUPS if any(k in name for k in keys)), 'other')
            by[grp] = by.get(grp, 0.0) + ns
            names.setdefault(grp, []).append((ns, name[:90]))
            tot += ns
    out = {'total_ms': round(tot / 1e6, 2), 'share': {g: round(v / tot, 4) for g, v in sorted(by.items(), key=lambda kv: -kv[1])},
           'largest_kernels': {g: [n for _, n in sorted(v, reverse=True)[:3]] for g, v in names.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=64)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=9, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--profile-only', action='store_true', help='run the bf16x3 model alone (the process to put under rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--shares', default=None, help='a *_kernel_stats.csv of such a run: print the kernel-time shares by family')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.shares:
        out = shares(a.shares)
    elif a.profile_only:
        profile_only(a)
        return
    else:
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
