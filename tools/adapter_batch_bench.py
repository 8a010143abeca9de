"""Cost of per-request LoRA adapters: d24 bf16 autoregressive_infer_cfg (incl. both decodes, the bench's sampling settings cfg 4, top_k 900,
top_p 0.96) eager at B = 512 and as one HIP graph at B = 8.  One model in one process, the modes interleaved call by call so that clock
and thermal drift fall on all alike:

  a  the per-request call on a model without a bank;
  b  the same call with a 4-adapter bank attached but no adapter= given (must be the same launches as a);
  c  adapter= all -1;
  d  four adapters mixed evenly over the batch;
  e  the alternative without a bank: four per-adapter sub-batches of B / 4, each on its own model with merged weights, one after the other.

Acceptance: b / a - 1 <= max(1 %, spread of a's repeats).  c / a, d / a and d / e are reported, no target.
--trace runs mode d alone a few times (eager, --trace-batch) for a `rocprofv3 --kernel-trace --stats` run of its own.

    python tools/adapter_batch_bench.py --out profiles/adapter_batch_d24.json
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
N_ADAPTERS, RANK = 4, 16


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


def adapter_state(var, seed, r=RANK, b_std=0.02):
    import torch
    from controlvar_amd import lora
    g = torch.Generator().manual_seed(seed)
    mods = dict(var.named_modules())
    sd = {}
    for t in lora.target_names(var):
        out_f, in_f = mods[t]._parameters['weight'].shape
        sd[f'{t}.lora_A.default.weight'] = (torch.rand(r, in_f, generator=g) * 2 - 1) / in_f ** 0.5
        sd[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * b_std
    return sd


def compare(B, calls, reps, warmup):
    """calls: {mode: fn(i)} -> per-mode medians, a's spread, the ratios and the verdict on b"""
    times = {m: [] for m in calls}
    modes = list(calls)
    for i in range(warmup):
        for m in modes:
            timed(lambda: calls[m](i))
    for i in range(reps):
        for m in modes[i % len(modes):] + modes[:i % len(modes)]:          # rotate the order call by call
            times[m].append(timed(lambda: calls[m](100 + i)))
    med = {m: statistics.median(v) for m, v in times.items()}
    res = {m: {'ms_median': round(med[m] * 1e3, 3), 'ms_all': [round(t * 1e3, 3) for t in times[m]], 'images_per_s': round(B / med[m], 2)} for m in calls}
    spread = (max(times['a']) - min(times['a'])) / med['a']
    bound = max(0.01, spread)
    res.update(a_spread=round(spread, 5), bound=round(bound, 5), b_over_a=round(med['b'] / med['a'], 5), within_bound=bool(med['b'] / med['a'] - 1.0 <= bound),
               c_over_a=round(med['c'] / med['a'], 5), d_over_a=round(med['d'] / med['a'], 5), d_over_e=round(med['d'] / med['e'], 5))
    return res


def run(a):
    import torch
    from controlvar_amd import lora, models
    dev = torch.device('cuda:0')
    bf = torch.bfloat16

    def build():
        vae = models.build_vae(compute_dtype=bf).to(dev)
        return models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()

    var = build()
    lora.attach_adapters(var, [adapter_state(var, 50 + k) for k in range(N_ADAPTERS)])
    bank = var._adapter_bank

    def with_bank(on):
        var._adapter_bank = bank if on else None            # mode a: the model as it is without a bank (nothing else differs)

    def rows(B, i):
        return dict(g_seed=[i] * B, cfg=[CFG] * B, top_k=[TOP_K] * B, top_p=[TOP_P] * B)

    if a.trace:
        B = a.trace_batch
        labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
        mixed = [b % N_ADAPTERS for b in range(B)]
        for i in range(3):
            var.autoregressive_infer_cfg(B, labels, cond_type=types, adapter=mixed, **rows(B, i))
        torch.cuda.synchronize()
        return None

    out = {'config': f'd{a.depth} ControlVAR autoregressive_infer_cfg 256^2 incl. both decodes, bf16, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; '
                     f'{N_ADAPTERS} adapters of rank {RANK}; modes a-e interleaved call by call in one process (see the tool), medians',
           'acceptance': 'b_over_a - 1 <= max(0.01, a_spread), a_spread = (max - min) / median of the repeats of a',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    # mode e: one model per adapter with W + s B A folded in
    merged = []
    for k in range(N_ADAPTERS):
        mk = build()
        mk.load_state_dict(lora.merged_adapter_state(var.state_dict(), bank, k))
        merged.append(mk)

    # ---- eager, the headline batch
    B = a.eager_batch
    q = B // N_ADAPTERS
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    mixed = [b % N_ADAPTERS for b in range(B)]

    def eager(on, **kw):
        def f(i):
            with_bank(on)
            try:
                var.autoregressive_infer_cfg(B, labels, cond_type=types, **rows(B, i), **kw)
            finally:
                with_bank(True)
        return f

    def eager_split(i):
        for k, mk in enumerate(merged):
            mk.autoregressive_infer_cfg(q, labels[k::N_ADAPTERS], cond_type=types[k::N_ADAPTERS], **rows(q, i))
            mk._arena = None                                # one K/V arena of B / 4 at a time: the block goes back to the allocator's cache for the next model

    calls = {'a': eager(False), 'b': eager(True), 'c': eager(True, adapter=-1), 'd': eager(True, adapter=mixed), 'e': eager_split}
    res = compare(B, calls, a.reps, a.warmup)
    out[f'eager_B{B}'] = res
    print(f'[adapter_batch] eager B={B}: ' + json.dumps(res), flush=True)

    # ---- captured, B = 8
    B = a.graph_batch
    q = B // N_ADAPTERS
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    mixed = [b % N_ADAPTERS for b in range(B)]
    kw = dict(cfg=CFG, top_k=TOP_K, top_p=TOP_P, per_request=True)
    with_bank(False)
    g_a = var.graphed_generator(B, **kw)
    with_bank(True)
    g_b = var.graphed_generator(B, **kw)
    g_ad = var.graphed_generator(B, adapters=True, **kw)
    g_e = [mk.graphed_generator(q, **kw) for mk in merged]

    def graph_split(i):
        for k, g in enumerate(g_e):
            g(labels[k::N_ADAPTERS], types[k::N_ADAPTERS], g_seed=[i] * q)

    calls = {'a': lambda i: g_a(labels, types, g_seed=[i] * B), 'b': lambda i: g_b(labels, types, g_seed=[i] * B),
             'c': lambda i: g_ad(labels, types, g_seed=[i] * B, adapter=-1), 'd': lambda i: g_ad(labels, types, g_seed=[i] * B, adapter=mixed), 'e': graph_split}
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    out[f'graph_B{B}'] = res
    print(f'[adapter_batch] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=512)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=10, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--trace', action='store_true', help='run mode d alone (eager, --trace-batch), for a kernel trace')
    ap.add_argument('--trace-batch', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 3 or a.graph_reps < 3:
        ap.error('at least three repeats per mode')
    if a.eager_batch % N_ADAPTERS or a.graph_batch % N_ADAPTERS:
        ap.error(f'batches must be multiples of {N_ADAPTERS}')
    out = run(a)
    if out is None:
        return
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
