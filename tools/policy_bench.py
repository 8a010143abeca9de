"""Cost of the token-level entrances of the d24 training step (bf16, B = 32, one GPU), one process, the three variants interleaved call by call so
that they see the same machine (the arrangement of tools/accum_bench.py):

  (a) step()                    on pixels: frozen tokenizer + forward + backward + clip + AdamW + W^T refresh
  (b) step_tokens()             supervised, on the ids of that tokenizer: (a) without the encoder and the quantiser
  (c) step_tokens(policy=...)   the clipped policy-gradient loss with ratio and KL term on (old_logprob, ref_logprob, kl_coef = 0.05):
                                cvar_pg_fwd_bwd in the place of cvar_ce_fwd_bwd, three (B, L) operands more

    python tools/policy_bench.py --out profiles/policy_d24.json

Expectations, written next to what was measured: (c) costs what (b) costs - within the larger of 1 % and the spread of (b)'s own
repeats; (b) is cheaper than (a) by about the tokenizer's share of the step.  One model, engine and optimizer serve all three (one set of
activations in HBM); every timed region ends in a device synchronise; token_logprobs, which a policy loop also pays per batch, is timed on its own."""
import argparse
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
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2, help='untimed rounds')
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    from controlvar_amd import models
    from controlvar_amd import train as T
    from controlvar_amd.synth import synth_images
    if not torch.cuda.is_available():
        raise SystemExit('policy_bench needs the GPU: nothing here can be timed without one')
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    B = a.batch
    vae = models.build_vae(compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev)
    tr = T.Trainer(var, vae, peak_lr=8e-5 * B / 512, weight_decay=0.08, sche='lin0', warmup_it=10, max_it=10000, clip=2.0, train_mode=True)
    g = torch.Generator().manual_seed(0)
    images, masks = synth_images(B, 256, seed=10).to(dev), synth_images(B, 256, seed=20).to(dev)
    cls, types = torch.randint(0, 1000, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
    both = vae.img_to_idxBl(torch.cat((masks, images), dim=0))
    ctrl, img = [t[:B].clone() for t in both], [t[B:].clone() for t in both]
    L = var.cfg.pyramid.L
    adv = torch.randn(B, generator=g).to(dev)
    ref = tr.token_logprobs(img, ctrl, cls, types, drop_seed=0).clone()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    t = {k: [] for k in ('pixels', 'tokens', 'policy', 'token_logprobs')}
    stats, seed = [], 0
    for r in range(a.warmup + a.rounds):
        rec = r >= a.warmup
        seed += 1
        ms_a, _ = timed(lambda: tr.step(images, masks, cls, types, drop_seed=seed, mask_first=True))
        ms_b, _ = timed(lambda: tr.step_tokens(img, ctrl, cls, types, drop_seed=seed))
        ms_l, old = timed(lambda: tr.token_logprobs(img, ctrl, cls, types, drop_seed=seed))
        pol = T.PolicyLoss(adv, old_logprob=old.clone(), ref_logprob=ref, clip=(0.2, 0.2), kl_coef=0.05)
        ms_c, o = timed(lambda: tr.step_tokens(img, ctrl, cls, types, policy=pol, drop_seed=seed))
        if rec:
            t['pixels'].append(ms_a); t['tokens'].append(ms_b); t['policy'].append(ms_c); t['token_logprobs'].append(ms_l)
            stats.append(dict(mean_ratio=round(o['mean_ratio'].item(), 6), clip_frac=round(o['clip_frac'].item(), 6), mean_kl=round(o['mean_kl'].item(), 6)))
    med = statistics.median
    base = med(t['tokens'])
    spread = (max(t['tokens']) - min(t['tokens'])) / base
    allowed = max(0.01, spread)
    out = {
        'config': f'd{a.depth} ControlVAR training step, bf16, B = {B}, L = {L}, train() mode, one GPU, one process, {a.rounds} interleaved rounds after '
                  f'{a.warmup} warm-up; host clock around a device synchronise',
        'lib_digest': lib_digest(),
        'a_step_pixels': dict(summary(t['pixels']), samples_per_s=round(B / med(t['pixels']) * 1e3, 2)),
        'b_step_tokens': dict(summary(t['tokens']), samples_per_s=round(B / base * 1e3, 2), spread_of_repeats=round(spread, 4)),
        'c_step_tokens_policy': dict(summary(t['policy']), samples_per_s=round(B / med(t['policy']) * 1e3, 2), last_rounds=stats[-3:]),
        'token_logprobs': summary(t['token_logprobs']),
        'policy_over_tokens': round(med(t['policy']) / base - 1, 4),
        'expected_policy_over_tokens': f'within max(1 %, spread of (b)) = {allowed:.4f}',
        'policy_within_expectation': bool(abs(med(t['policy']) / base - 1) <= allowed),
        'tokens_saving_over_pixels': round(1 - base / med(t['pixels']), 4),
        'expected_tokens_saving': 'about the tokenizer share of the step (6.6 % of its flops, plus the image input)',
        'note': 'the model keeps its condition dropout (cond_drop_rate 0.1, drawn per forward outside drop_seed) and the optimizer moves between the '
                'reference and the step, so the ratio and KL figures of last_rounds are far from 1 and 0: they show that the terms are live, no more',
        'mem_GB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
