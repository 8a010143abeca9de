"""What top_logprobs=N and the sparse distillation targets cost on d24 (bf16, one GPU), one process, the variants of every comparison interleaved call
by call so that they see the same machine (the arrangement of tools/distill_bench.py):

  (a) generation:     the per-request joint call with logprobs=True against the same call with top_logprobs=N: eager at B = 512, one HIP graph at B = 8
  (b) training step:  step_tokens(distill=dense) against step_tokens(distill=sparse, N) at B = 32, and the bytes of the stored targets

    python tools/topn_bench.py --out profiles/topn_d24.json

Expectations are written in DESIGN.md 8e before the numbers; every timed region ends in a device synchronise (host clock), medians and ranges over
the rounds after the warm-up."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2), 'n': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--topn', type=int, default=32)
    ap.add_argument('--train-batch', type=int, default=32)
    ap.add_argument('--joint-batch', type=int, default=512)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--train-rounds', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=4, help='timed eager generation calls per variant')
    ap.add_argument('--graph-rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1, help='untimed rounds')
    ap.add_argument('--skip', default='', help="comma list of 'train', 'eager', 'graph'")
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    from controlvar_amd import models, ops
    from controlvar_amd import train as T
    from controlvar_amd.synth import synth_images
    if not torch.cuda.is_available():
        raise SystemExit('topn_bench needs the GPU: nothing here can be timed without one')
    dev, bf, N = torch.device('cuda:0'), torch.bfloat16, a.topn
    skip = set(filter(None, a.skip.split(',')))
    med = statistics.median

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    out = {'config': f'd{a.depth} ControlVAR, bf16, one GPU, one process, N = {N}, interleaved call by call after {a.warmup} warm-up; host clock around a '
                     'device synchronise'}

    def pair(name, B, variants, rounds, unit):
        t = {k: [] for k in variants}
        for r in range(a.warmup + rounds):
            for k, fn in variants.items():
                ms, _ = timed(lambda: fn(r))
                if r >= a.warmup:
                    t[k].append(ms)
        (k0, t0), (k1, t1) = t.items()
        out[name] = {'B': B, k0: dict(summary(t0), **{unit: round(B / med(t0) * 1e3, 2)}), k1: dict(summary(t1), **{unit: round(B / med(t1) * 1e3, 2)}),
                     f'{k1}_over_{k0}_time': round(med(t1) / med(t0), 4), 'spread_of_' + k0: round((max(t0) - min(t0)) / med(t0), 4)}
        print(f'[topn_bench] {name}: {json.dumps(out[name])}', file=sys.stderr, flush=True)

    vae = models.build_vae(compute_dtype=bf).to(dev)
    g = torch.Generator().manual_seed(0)

    if 'train' not in skip:
        B = a.train_batch
        var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf, cond_drop_rate=0.0).to(dev)
        tr = T.Trainer(var, vae, peak_lr=8e-5 * B / 512, weight_decay=0.08, sche='lin0', warmup_it=10, max_it=10000, clip=2.0, train_mode=True)
        images, masks = synth_images(B, 256, seed=10).to(dev), synth_images(B, 256, seed=20).to(dev)
        cls, types = torch.randint(0, 1000, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
        both = vae.img_to_idxBl(torch.cat((masks, images), dim=0))
        ctrl, img = [t[:B].clone() for t in both], [t[B:].clone() for t in both]
        L, V = var.cfg.pyramid.L, var.cfg.vocab
        teacher = (torch.randn(B, L, V, device=dev) * 3.0).contiguous()          # the cost does not depend on the values
        ids = torch.empty(B, L, N, dtype=torch.int32, device=dev)
        lp, tail = torch.empty(B, L, N, device=dev), torch.empty(B, L, device=dev)
        ops.score_topn(teacher, B, 1, L, V, torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(B, 1), N, ids, lp, tail)
        dense, sparse = T.DistillLoss(teacher), T.SparseDistillLoss(ids, lp, tail)
        pair('train', B, {'dense': lambda r: tr.step_tokens(img, ctrl, cls, types, distill=dense, drop_seed=r),
                          'sparse': lambda r: tr.step_tokens(img, ctrl, cls, types, distill=sparse, drop_seed=r)}, a.train_rounds, 'samples_per_s')
        sb = ids.numel() * 4 + lp.numel() * 4 + tail.numel() * 4
        out['train']['target_bytes_per_sample'] = {'dense': L * V * 4, 'sparse': sb // B, 'dense_over_sparse': round(L * V * 4 * B / sb, 1)}
        del tr, var, teacher, dense, sparse
        gc.collect(); torch.cuda.empty_cache()

    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    kw = dict(top_k=900, top_p=0.96)

    def labels(B):
        return torch.randint(0, 1000, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)

    if 'eager' not in skip:
        B = a.joint_batch
        lab, ty = labels(B)
        pair('joint_eager', B, {'logprobs': lambda r: var.autoregressive_infer_cfg(B, lab, g_seed=r, cfg=4.0, cond_type=ty, logprobs=True, **kw),
                                'top_logprobs': lambda r: var.autoregressive_infer_cfg(B, lab, g_seed=r, cfg=4.0, cond_type=ty, logprobs=True, top_logprobs=N, **kw)},
             a.rounds, 'images_per_s')
    if 'graph' not in skip:
        var._arena = None
        gc.collect(); torch.cuda.empty_cache()
        B = a.graph_batch
        lab, ty = labels(B)
        g0 = var.graphed_generator(B, cfg=4.0, per_request=True, logprobs=True, **kw)
        g1 = var.graphed_generator(B, cfg=4.0, per_request=True, logprobs=True, top_logprobs=N, **kw)
        pair('joint_graph', B, {'logprobs': lambda r: g0(lab, ty, g_seed=r), 'top_logprobs': lambda r: g1(lab, ty, g_seed=r)}, a.graph_rounds, 'images_per_s')
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
