"""Generation rate of the d36 model (C = 2304, 36 heads, VAR(shared_aln=True) on PATCH_NUMS_512: 512 x 512 images, 2 240 tokens) beside the d30 model at
the same settings.

One process, one GPU, bf16, autoregressive_infer_cfg incl. the decode (ch 160 VQVAE) with cfg 4, top_k 900, top_p 0.96: one HIP graph at the batches of
`--graph` (default 1 and 8), eager calls at the batches of `--eager` (default 32); warm-up plus `--reps` timed calls each, median / min / max, images/s and
torch's peak allocated memory of the entry.  A batch that does not fit is recorded as such.  The weights are synthetic (controlvar_amd.synth): no published
d36 checkpoint is loaded.  Nothing is asserted: there is no earlier number at this width; the file is the record.

    python tools/wide_bench.py --out profiles/wide_d36.json
    python tools/wide_bench.py --depth 36 --eager 8 --graph --reps 3         # one short eager entry, e.g. under a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats_ms(v):
    return {'ms_median': round(statistics.median(v), 3), 'ms_min': round(min(v), 3), 'ms_max': round(max(v), 3), 'n': len(v)}


def timed(torch, call, a):
    def one(i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for i in range(a.warmup):
        one(i)
    return [one(100 + i) for i in range(a.reps)]


def entry(torch, var, B, graph, a):
    kw = dict(cfg=4.0, top_k=900, top_p=0.96)
    labels = torch.arange(B) % 1000
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    try:
        if graph:
            run = var.graphed_generator(B, **kw)
            ms = timed(torch, lambda i: run(labels, g_seed=i), a)
            del run
        else:
            ms = timed(torch, lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=i, **kw), a)
        res = stats_ms(ms)
        res.update(B=B, mode='graph' if graph else 'eager', images_per_s=round(B / statistics.median(ms) * 1e3, 3),
                   peak_mem_GB=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                   kv_arena_GB=round(sum(t.numel() * t.element_size() for _, t in (var._arena or {}).values()) / 2 ** 30, 2))
    except torch.cuda.OutOfMemoryError:
        res = {'B': B, 'mode': 'graph' if graph else 'eager', 'error': 'out of memory'}
    var._arena = None
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, nargs='+', default=[36, 30])
    ap.add_argument('--graph', type=int, nargs='*', default=[1, 8])
    ap.add_argument('--eager', type=int, nargs='*', default=[32])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from controlvar_amd import models
    from controlvar_amd.spec import PATCH_NUMS_512
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    out = {'config': 'VAR(shared_aln=True), PATCH_NUMS_512, autoregressive_infer_cfg incl. the decode (ch 160 VQVAE), bf16, cfg 4, top_k 900, top_p 0.96, one GPU; '
                     f'{a.warmup} warm-up + {a.reps} timed calls per entry, wall clock around a synchronised call; synthetic weights',
           'device': torch.cuda.get_device_name(dev), 'models': {}}
    vae = models.build_vae(compute_dtype=bf, v_patch_nums=PATCH_NUMS_512).to(dev)
    for depth in a.depth:
        t0 = time.perf_counter()
        print(f'[wide_bench] building d{depth} (synthetic weights on the host) ...', flush=True)
        var = models.build_var(vae, depth=depth, shared_aln=True, patch_nums=PATCH_NUMS_512, compute_dtype=bf).to(dev).eval()
        m = {'embed_dim': var.C, 'heads': var.num_heads, 'parameters_G': round(sum(p.numel() for p in var.parameters()) / 1e9, 3),
             'build_s': round(time.perf_counter() - t0, 1), 'entries': []}
        for graph, batches in ((True, a.graph), (False, a.eager)):
            for B in batches:
                res = entry(torch, var, B, graph, a)
                m['entries'].append(res)
                print(f'[wide_bench] d{depth} ' + json.dumps(res), flush=True)
        out['models'][f'd{depth}'] = m
        del var
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
