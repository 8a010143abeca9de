"""What kv_precision='fp8' costs and buys: d24 ControlVAR 256^2 incl. both decodes, the bench's sampling settings (cfg 4, top_k 900, top_p 0.96), the
two modes interleaved call by call in one process so that clock and thermal drift fall on both alike:

    bf16   compute_dtype=bfloat16                          (throughput mode) - the baseline of the comparison, the same build
    kv8    compute_dtype=bfloat16, kv_precision='fp8'      (the bf16 model over an e4m3 K/V arena with per-(token, head) scales: 17/32 of the bytes)

Eager at --eager-batch (default 512, the headline batch) and as one HIP graph at --graph-batch (8).  The bf16 arena at B = 512 is 205 GB, the e4m3 one
109 GB: the two do not fit side by side, so every eager call first drops both models' arenas, empties the allocator's cache and allocates the call's own
arena (all untimed): no device allocation of 100+ GB falls into the timed region of either mode.  Reports per mode ms and images/s, the spread of the bf16 baseline's repeats, the
ratio bf16 / kv8 and torch.cuda.max_memory_allocated of one generation of each mode.

This is a capacity feature: the ratio is reported as it comes out, there is no acceptance threshold.

B = --big-batch (1024): one generation in the kv8 mode, only if its size - the e4m3 arena computed from the shapes plus everything else, taken as
(big / eager) x what the kv8 generation at --eager-batch peaked at beyond its own arena and the weights - stays below 0.9 of the free memory.  The
limit is never found by trying: otherwise the record says "not run" with the computed size.

Where the time goes comes from a run of its own (tracing slows the host; never combined with the timing above):

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/kv8_bench.py --profile-only [--profile-mode bf16]
    python tools/kv8_bench.py --shares OUT/.../*_kernel_stats.csv          # append pass / attention / GEMMs / decoder / other

    python tools/kv8_bench.py --out profiles/kv8_d24.json
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
MODES = ('bf16', 'kv8')
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
    """calls: {mode: fn(i)} -> per-mode medians, the baseline's spread and the ratio.  before(mode): untimed preparation of a call"""
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
    gain = med[BASE] / med['kv8']
    res.update(baseline_spread=round(spread, 5), bf16_over_kv8=round(gain, 4), kv8_is_slower=bool(gain < 1.0))
    return res


def build(depth, dev, modes=MODES):
    import torch
    from controlvar_amd import models
    out = {}
    for mode in modes:
        vae = models.build_vae(compute_dtype=torch.bfloat16).to(dev)
        m = models.build_control_var(vae, depth=depth, mask_type='interleave_append', multi_cond=True, compute_dtype=torch.bfloat16,
                                     kv_precision='fp8' if mode == 'kv8' else None).to(dev).eval()
        m._pack(); vae._pack()
        torch.cuda.synchronize()
        out[mode] = m
    return out


def arena_bytes(m, B, mode):
    """bytes of the K/V arena of a B-image generation (R = 2B sequences), from the shapes"""
    from controlvar_amd import models
    cfg = m.cfg
    if mode == 'kv8':
        sq, ss = models.kv8_arena_shapes(cfg.depth, 2 * B, cfg.pyramid.L, cfg.H)
        n = 4
        for d in ss:
            n *= d
        q = 1
        for d in sq:
            q *= d
        return q + n
    return cfg.depth * 2 * B * cfg.pyramid.L * 2 * cfg.C * 2


def run(a):
    import torch
    dev = torch.device('cuda:0')
    var = build(a.depth, dev)
    out = {'config': f'd{a.depth} ControlVAR 256^2 incl. both decodes, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; autoregressive_infer_cfg of two bf16 models '
                     '(kv_precision None / fp8) interleaved call by call in one process, median of the timed calls of each',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    def drop_arenas(mode=None, batch=None):
        for m in var.values():
            m._arena = None
        torch.cuda.empty_cache()
        if mode is not None and batch:                   # the call's own arena, allocated here: no device allocation of 100+ GB in the timed region
            var[mode]._get_arena(2 * batch, var[mode].cfg.pyramid.L, var[mode].kv_precision)

    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    calls = {m: (lambda i, m=m: var[m].autoregressive_infer_cfg(B, labels, g_seed=i, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=types)) for m in MODES}
    res = compare(B, calls, a.reps, a.warmup, before=lambda m: drop_arenas(m, B))
    out[f'eager_B{B}'] = res
    print(f'[kv8_bench] eager B={B}: ' + json.dumps(res), flush=True)

    # ---- peak memory of one generation of each mode, from an empty cache
    mem = {}
    drop_arenas()
    weights = torch.cuda.memory_allocated(dev)
    for m in MODES:
        drop_arenas()
        torch.cuda.reset_peak_memory_stats(dev)
        calls[m](7)
        torch.cuda.synchronize()
        mem[m] = {'max_memory_allocated': torch.cuda.max_memory_allocated(dev), 'arena_bytes': arena_bytes(var[m], B, m)}
    drop_arenas()
    mem['resident_before_a_generation'] = weights
    mem['kv8_over_bf16_peak'] = round(mem['kv8']['max_memory_allocated'] / mem['bf16']['max_memory_allocated'], 4)
    out[f'memory_B{B}'] = mem
    print(f'[kv8_bench] memory B={B}: ' + json.dumps(mem), flush=True)

    # ---- one generation at the big batch, kv8 only, if the computed size allows it
    BB = a.big_batch
    free, total = torch.cuda.mem_get_info(dev)
    rest = mem['kv8']['max_memory_allocated'] - mem['kv8']['arena_bytes'] - weights            # everything else of the B = eager-batch generation
    need = arena_bytes(var['kv8'], BB, 'kv8') + rest * BB // B
    big = {'computed_bytes': need, 'free_bytes': free, 'limit': 0.9, 'arena_bytes': arena_bytes(var['kv8'], BB, 'kv8'),
           'bf16_arena_bytes_would_be': arena_bytes(var['bf16'], BB, 'bf16')}
    if need < 0.9 * free:
        lb, tb = torch.arange(BB) % 1000, torch.arange(BB) % 4
        torch.cuda.reset_peak_memory_stats(dev)
        t = timed(lambda: var['kv8'].autoregressive_infer_cfg(BB, lb, g_seed=1, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=tb))       # cold: includes the arena's allocation
        t = min(t, timed(lambda: var['kv8'].autoregressive_infer_cfg(BB, lb, g_seed=2, cfg=CFG, top_k=TOP_K, top_p=TOP_P, cond_type=tb)))
        big.update(ran=True, ms=round(t * 1e3, 3), images_per_s=round(BB / t, 2), max_memory_allocated=torch.cuda.max_memory_allocated(dev))
    else:
        big.update(ran=False, note='not run: the computed size is not below 0.9 of the free memory')
    out[f'big_B{BB}'] = big
    print(f'[kv8_bench] B={BB}: ' + json.dumps(big), flush=True)
    drop_arenas()

    B = a.graph_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    graphs = {m: var[m].graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P) for m in MODES}
    calls = {m: (lambda i, m=m: graphs[m](labels, types, g_seed=i)) for m in MODES}
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    out[f'graph_B{B}'] = res
    print(f'[kv8_bench] graph B={B}: ' + json.dumps(res), flush=True)
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
    print(f'[kv8_bench] profile-only: two {a.profile_mode} generations at B={B} done', flush=True)


GROUPS = (('kv_append_fp8', ('kv_append_fp8_kernel',)), ('attention', ('attn_', 'cos_qk_norm')),
          ('decoder_and_quantizer', ('conv3x3', 'conv_', 'gn_', 'softmax_rows', 'transpose_kernel', 'ms_', 'ms32', 'resample_sep', 'embed_rows', 'nchw', 'nhwc', 'rowsum')),
          ('gemm_bf16', ('cvar_gemm', 'cvar_splitk')), ('ln_modulate', ('ln_modulate',)), ('sampler', ('cfg_',)))


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
    ap.add_argument('--big-batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=9, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--profile-only', action='store_true', help='run one model alone (the process to put under rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--profile-mode', choices=MODES, default='kv8')
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
