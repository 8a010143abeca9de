"""What guidance distillation costs and saves on d24 (bf16, one GPU), one process, the variants of every comparison interleaved call by call so that they
see the same machine (the arrangement of tools/policy_bench.py):

  (i)  training step, B = 32:   step_tokens() supervised against step_tokens(distill=...) - cvar_kd_fwd_bwd in the place of cvar_ce_fwd_bwd, and
                                three reads of M * V * 4 bytes of teacher logits more
  (ii) generation:              the guided call against cfg=None (no guidance rows), for autoregressive_infer_cfg (2 B rows against B) and
                                conditional_infer_cfg with the control given (4 B rows against B): eager at a large batch, one HIP graph at B = 8;
                                peak memory of each eager call

    python tools/distill_bench.py --out profiles/distill_d24.json

The eager joint call runs at B = 512 (the headline batch).  The eager conditional call runs at B = 128: its guided form holds 4 B sequences in the K/V
arena, which at B = 512 would be 410 GB.  Expectations are written in DESIGN.md 8e before the numbers; every timed region ends in a device synchronise
(host clock), medians and ranges over the rounds after the warm-up.  The eager variants alternate in blocks (see pair()), the graphs and the training
steps call by call."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lib_digest():
    try:
        return open(os.path.join(ROOT, 'controlvar_amd', 'csrc', 'build', 'digest.txt')).read().strip()[:16]
    except OSError:
        return None


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2), 'n': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--train-batch', type=int, default=32)
    ap.add_argument('--joint-batch', type=int, default=512)
    ap.add_argument('--cond-batch', type=int, default=128)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=3, help='timed eager calls per block (two blocks per variant)')
    ap.add_argument('--graph-rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1, help='untimed rounds')
    ap.add_argument('--skip', default='', help="comma list of 'train', 'eager', 'graph'")
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    from controlvar_amd import models
    from controlvar_amd import train as T
    from controlvar_amd.synth import synth_images
    if not torch.cuda.is_available():
        raise SystemExit('distill_bench needs the GPU: nothing here can be timed without one')
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    skip = set(filter(None, a.skip.split(',')))
    med = statistics.median

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    out = {'config': f'd{a.depth} ControlVAR, bf16, one GPU, one process, interleaved rounds after {a.warmup} warm-up; host clock around a device synchronise',
           'lib_digest': lib_digest()}
    vae = models.build_vae(compute_dtype=bf).to(dev)
    g = torch.Generator().manual_seed(0)

    # ---- (i) the training step
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
        dl = T.DistillLoss(teacher)
        t = {'tokens': [], 'distill': []}
        for r in range(a.warmup + 8):
            ms_b, _ = timed(lambda: tr.step_tokens(img, ctrl, cls, types, drop_seed=r))
            ms_c, o = timed(lambda: tr.step_tokens(img, ctrl, cls, types, distill=dl, drop_seed=r))
            if r >= a.warmup:
                t['tokens'].append(ms_b); t['distill'].append(ms_c)
        base = med(t['tokens'])
        spread = (max(t['tokens']) - min(t['tokens'])) / base
        allowed = max(0.01, spread)
        out['train'] = {
            'what': f'B = {B}, L = {L}, train() mode; teacher logits {B} x {L} x {V} fp32 = {B * L * V * 4 / 2 ** 30:.2f} GiB, read three times',
            'step_tokens': dict(summary(t['tokens']), samples_per_s=round(B / base * 1e3, 2), spread_of_repeats=round(spread, 4)),
            'step_tokens_distill': dict(summary(t['distill']), samples_per_s=round(B / med(t['distill']) * 1e3, 2), last_kl=round(float(o['loss']), 4)),
            'distill_over_tokens': round(med(t['distill']) / base - 1, 4),
            'expected': f'within max(1 %, spread of step_tokens) = {allowed:.4f}',
            'within_expectation': bool(abs(med(t['distill']) / base - 1) <= allowed),
            'mem_GB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
        }
        print(f"[distill_bench] train: {json.dumps(out['train'])}", file=sys.stderr, flush=True)
        del tr, var, teacher, dl
        gc.collect(); torch.cuda.empty_cache()

    # ---- (ii) generation
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    kw = dict(top_k=900, top_p=0.96)

    def pair(name, B, guided, unguided, rounds, mem=True):
        """graphs (mem=False): the two variants alternate call by call.  Eager calls (mem=True) alternate in blocks - guided, unguided, guided,
        unguided, each block the warm-up and rounds timed calls: the two K/V arenas do not fit side by side at the large batch, so every change of
        variant frees one arena and allocates the other, and that (seconds for 200 GB) belongs to the block's untimed warm-up, not to a call"""
        t, peak = {'guided': [], 'unguided': []}, {}
        if mem:
            for _ in range(2):
                for k, fn in (('guided', guided), ('unguided', unguided)):
                    var._arena = None
                    gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                    for r in range(a.warmup + rounds):
                        ms, _ = timed(lambda: fn(r))
                        if r >= a.warmup:
                            t[k].append(ms)
                    peak[k] = max(peak.get(k, 0.0), torch.cuda.max_memory_allocated() / 2 ** 30)
        else:
            for r in range(a.warmup + rounds):
                for k, fn in (('guided', guided), ('unguided', unguided)):
                    ms, _ = timed(lambda: fn(r))
                    if r >= a.warmup:
                        t[k].append(ms)
        gm, um = med(t['guided']), med(t['unguided'])
        out[name] = {'B': B, 'guided': dict(summary(t['guided']), images_per_s=round(B / gm * 1e3, 2)),
                     'unguided': dict(summary(t['unguided']), images_per_s=round(B / um * 1e3, 2)), 'unguided_over_guided_time': round(um / gm, 4),
                     'speedup': round(gm / um, 3)}
        if mem:
            out[name]['peak_mem_GB'] = {k: round(v, 1) for k, v in peak.items()}
        print(f'[distill_bench] {name}: {json.dumps(out[name])}', file=sys.stderr, flush=True)

    def labels(B):
        return torch.randint(0, 1000, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)

    if 'eager' not in skip:
        B = a.joint_batch
        lab, ty = labels(B)
        pair('joint_eager', B, lambda r: var.autoregressive_infer_cfg(B, lab, g_seed=r, cfg=4.0, cond_type=ty, **kw),
             lambda r: var.autoregressive_infer_cfg(B, lab, g_seed=r, cfg=None, cond_type=ty, **kw), a.rounds)
        B = a.cond_batch
        lab, ty = labels(B)
        given = [t.clone() for t in vae.img_to_idxBl(synth_images(B, 256, seed=30).to(dev))]
        pair('conditional_eager', B, lambda r: var.conditional_infer_cfg(B, lab, g_seed=r, cfg=(4.0, 4.0, 4.0), cond_type=ty, c_mask=given, **kw),
             lambda r: var.conditional_infer_cfg(B, lab, g_seed=r, cfg=None, cond_type=ty, c_mask=given, **kw), a.rounds)
        del given
    if 'graph' not in skip:
        var._arena = None
        gc.collect(); torch.cuda.empty_cache()
        B = a.graph_batch
        lab, ty = labels(B)
        given = [t.clone() for t in vae.img_to_idxBl(synth_images(B, 256, seed=31).to(dev))]
        g2, g1 = var.graphed_generator(B, cfg=4.0, **kw), var.graphed_generator(B, cfg=None, **kw)
        pair('joint_graph', B, lambda r: g2(lab, ty, g_seed=r), lambda r: g1(lab, ty, g_seed=r), a.graph_rounds, mem=False)
        del g2, g1
        c4, c1 = var.graphed_conditional_generator(B, cfg=(4.0, 4.0, 4.0), **kw), var.graphed_conditional_generator(B, cfg=None, **kw)
        pair('conditional_graph', B, lambda r: c4(lab, ty, given, g_seed=r), lambda r: c1(lab, ty, given, g_seed=r), a.graph_rounds, mem=False)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
