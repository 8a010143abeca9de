"""What gemm_precision='fp8' costs and buys: d24 ControlVAR 256^2 incl. both decodes, the bench's sampling settings (cfg 4, top_k 900, top_p 0.96), the
two modes interleaved call by call in one process so that clock and thermal drift fall on both alike:

    bf16   compute_dtype=bfloat16                          (throughput mode) - the baseline of the comparison, the same build
    fp8    compute_dtype=bfloat16, gemm_precision='fp8'    (the bf16 model, qkv / proj / fc1 / fc2 on e4m3 operands)

Eager at --eager-batch (default 512, the headline batch) and as one HIP graph at --graph-batch (8).  The K/V arena of a d24 bf16 model at B = 512 is 205 GB:
the two models cannot hold one each, so every eager call first drops the OTHER model's arena - the block goes back to torch's caching allocator and the
call's own arena is that block again, no device allocation in the timed region.  Reports per mode ms and images/s, the spread of the bf16 baseline's repeats and
the ratio bf16 / fp8.

The one condition: fp8 beats bf16 by more than the larger of 1 % and the baseline's spread (`fp8_beats_bf16`); the figure is reported either way.

A kernel-time breakdown of the mode comes from a run of its own (tracing slows the host; never combined with the timing above):

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/fp8_bench.py --profile-only
    python tools/fp8_bench.py --shares OUT/.../*_kernel_stats.csv          # fp8 GEMMs / the two quantiser kernels / bf16 GEMMs / attention / decoder / other

    python tools/fp8_bench.py --out profiles/fp8_d24.json
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
MODES = ('bf16', 'fp8')
BASE = 'bf16'


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


def compare(B, calls, reps, warmup, before=None):
    """calls: {mode: fn(i)} -> per-mode medians, the baseline's spread, the ratio and the verdict.  before(mode): untimed preparation of a call"""
    modes = list(calls)
    times = {m: [] for m in modes}
    for i in range(warmup):
        for m in modes:
            if before:
                before(m)
            timed(lambda: calls[m](i))
    for i in range(reps):
        for m in modes[i % len(modes):] + modes[:i % len(modes)]:           # rotate the order: no mode always runs behind the same one
            if before:
                before(m)
            times[m].append(timed(lambda: calls[m](100 + i)))
    med = {m: statistics.median(v) for m, v in times.items()}
    res = {m: {'ms_median': round(med[m] * 1e3, 3), 'ms_all': [round(t * 1e3, 3) for t in times[m]], 'images_per_s': round(B / med[m], 2)} for m in modes}
    spread = (max(times[BASE]) - min(times[BASE])) / med[BASE]
    bound = max(0.01, spread)
    gain = med[BASE] / med['fp8']
    res.update(baseline_spread=round(spread, 5), bound=round(bound, 5), bf16_over_fp8=round(gain, 4), fp8_beats_bf16=bool(gain - 1.0 > bound))
    return res


def build(depth, dev, modes=MODES):
    import torch
    from controlvar_amd import models
    out = {}
    for mode in modes:
        vae = models.build_vae(compute_dtype=torch.bfloat16).to(dev)
        m = models.build_control_var(vae, depth=depth, mask_type='interleave_append', multi_cond=True, compute_dtype=torch.bfloat16,
                                     gemm_precision='fp8' if mode == 'fp8' else None).to(dev).eval()
        m._pack(); vae._pack()
        torch.cuda.synchronize()
        out[mode] = m
    return out


def run(a):
    import torch
    dev = torch.device('cuda:0')
    var = build(a.depth, dev)
    out = {'config': f'd{a.depth} ControlVAR 256^2 incl. both decodes, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; autoregressive_infer_cfg of two bf16 models '
                     '(gemm_precision None / fp8) interleaved call by call in one process, median of the timed calls of each',
           'acceptance': 'bf16_over_fp8 - 1 > max(0.01, baseline_spread), baseline_spread = (max - min) / median of the bf16 repeats',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    def drop_other_arena(mode):
        for k, m in var.items():
            if k != mode:
                m._arena = None

    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    calls = {m: (lambda i, m=m: var[m].autoregressive_infer_cfg(B, labels, g_seed=i, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types)) for m in MODES}
    res = compare(B, calls, a.reps, a.warmup, before=drop_other_arena)
    out[f'eager_B{B}'] = res
    print(f'[fp8_bench] eager B={B}: ' + json.dumps(res), flush=True)
    for m in MODES:
        var[m]._arena = None
    torch.cuda.empty_cache()

    B = a.graph_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    graphs = {m: var[m].graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P) for m in MODES}
    calls = {m: (lambda i, m=m: graphs[m](labels, types, g_seed=i)) for m in MODES}
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    out[f'graph_B{B}'] = res
    print(f'[fp8_bench] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def profile_only(a):
    """one model alone (--profile-mode), one warm-up and one generation at --eager-batch: the process rocprofv3 traces"""
    import torch
    dev = torch.device('cuda:0')
    m = build(a.depth, dev, modes=(a.profile_mode,))[a.profile_mode]
    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    for i in range(2):
        m.autoregressive_infer_cfg(B, labels, g_seed=i, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types)
    torch.cuda.synchronize()
    print(f'[fp8_bench] profile-only: two {a.profile_mode} generations at B={B} done', flush=True)


# the adaLN kernel with the e4m3 store carries fp8q_t in its name; the bf16 GEMMs left in this mode are the head, the adaLN table and the VQVAE's
GROUPS = (('gemm_fp8', ('cvar_gemm_fp8_kernel',)), ('quant_rows_fp8', ('quant_rows_fp8_kernel',)), ('ln_modulate_fp8', ('fp8q_t',)),
          ('decoder_and_quantizer', ('conv3x3', 'conv_', 'gn_', 'softmax_rows', 'transpose_kernel', 'ms_', 'ms32', 'resample_sep', 'embed_rows', 'nchw', 'nhwc', 'rowsum')),
          ('gemm_bf16', ('cvar_gemm', 'cvar_splitk')), ('attention', ('attn_', 'cos_qk_norm')), ('ln_modulate_bf16', ('ln_modulate',)), ('sampler', ('cfg_',)))


def shares(path):
    """kernel-time shares of a rocprofv3 --stats csv by kernel family (names matched in the order of GROUPS)"""
    tot, by, names = 0.0, {}, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            ns = float(row.get('TotalDurationNs') or row.get('TotalDuration(ns)') or 0)
            grp = next((g for g, keys in GROUPS if any(k in name for k in keys)), 'other')
            by[grp] = by.get(grp, 0.0) + ns
            names.setdefault(grp, []).append((ns, name[:90]))
            tot += ns
    return {'total_ms': round(tot / 1e6, 2), 'ms': {g: round(v / 1e6, 2) for g, v in sorted(by.items(), key=lambda kv: -kv[1])},
            'share': {g: round(v / tot, 4) for g, v in sorted(by.items(), key=lambda kv: -kv[1])},
            'largest_kernels': {g: [n for _, n in sorted(v, reverse=True)[:3]] for g, v in names.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=512)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=9, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--profile-only', action='store_true', help='run one model alone (the process to put under rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--profile-mode', choices=MODES, default='fp8')
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
