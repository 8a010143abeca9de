"""The policy-gradient loop closed once - a demonstration on the synthetic weights, not a result and not a test:

  sample     G images per (class, control type) with autoregressive_infer_cfg(..., logprobs=True) on a LoRA model; the drawn ids are the
             trace of the generation, split per scale into their control and image halves
  reward     a toy: mean brightness of the image half (the lower half of the returned pair)
  advantage  group-normalised: (reward - mean of its group) / (std of its group + eps)
  reference  Trainer.token_logprobs before the first update: ref_logprob of the KL term and old_logprob of the ratio
  update     a few Trainer.step_tokens(policy=PolicyLoss(...)) on the sampled batch; from the second one on the ratio leaves 1 and clips

    python tools/grpo_demo.py --depth 2 --groups 2 --group-size 4 --iters 4

The ratio is taken between training forwards (the scoring forward of token_logprobs is the training forward), so it is exactly 1.0 in the
first update whatever guidance and filters the sampler used."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--groups', type=int, default=2)
    ap.add_argument('--group-size', type=int, default=4)
    ap.add_argument('--iters', type=int, default=4, help='policy steps on the sampled batch')
    ap.add_argument('--lr', type=float, default=2e-3)
    ap.add_argument('--kl', type=float, default=0.02)
    a = ap.parse_args()
    import torch
    from controlvar_amd import lora, models
    from controlvar_amd import train as T
    if not torch.cuda.is_available():
        raise SystemExit('grpo_demo needs the GPU')
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(ch=32 if a.depth <= 4 else 160, compute_dtype=bf).to(dev)
    m = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf, cond_drop_rate=0.0).to(dev)
    lora.add_lora(m, r=16, dropout=0.0, seed=1)
    tr = T.Trainer(m, vae, peak_lr=a.lr, weight_decay=0.0, sche='lin0', warmup_it=0, max_it=1000, clip=2.0, drop_path=False, train_mode=False)
    G, n = a.group_size, a.groups
    B = G * n
    g = torch.Generator().manual_seed(0)
    cls = torch.randint(0, 1000, (n,), generator=g).repeat_interleave(G)
    types = torch.randint(0, 4, (n,), generator=g).repeat_interleave(G)
    pns = m.cfg.pyramid.patch_nums

    def sample(seed):           # one seed per row: identical requests with one seed would draw identical samples and every advantage would be 0
        images, scores = m.autoregressive_infer_cfg(B, cls, g_seed=[seed * 1000 + b for b in range(B)], cfg=1.5, top_k=900, top_p=0.96, cond_type=types, _trace=True, logprobs=True)
        idx = [t[:B].long() for t in m.last_trace['idx']]                          # per scale (B, 2 pn^2): control half, then image half
        H = images.shape[2] // 2
        reward = images[:, :, H:].float().mean(dim=(1, 2, 3))                      # brightness of the RGB half
        return [t[:, :pn * pn] for t, pn in zip(idx, pns)], [t[:, pn * pn:] for t, pn in zip(idx, pns)], reward, scores

    ctrl, img, reward, scores = sample(100)
    r = reward.view(n, G)
    adv = ((r - r.mean(1, keepdim=True)) / (r.std(1, keepdim=True) + 1e-6)).view(B)
    print(f'[grpo] sampled {n} groups of {G}: reward {reward.mean().item():.4f}, sampler log-probability per token {scores.logprob.mean().item():.3f}')
    ref = old = tr.token_logprobs(img, ctrl, cls, types).clone()                   # before the first update: the reference policy and the old policy
    for u in range(a.iters):
        o = tr.step_tokens(img, ctrl, cls, types, policy=T.PolicyLoss(adv, old_logprob=old, ref_logprob=ref, clip=(0.2, 0.2), kl_coef=a.kl))
        print(f'[grpo] update {u}: loss {o["loss"].item():+.5f}  ratio {o["mean_ratio"].item():.4f}  clipped {o["clip_frac"].item():.3f}  '
              f'kl {o["mean_kl"].item():.2e}  grad_norm {o["grad_norm"].item():.3f}')
    lp = tr.token_logprobs(img, ctrl, cls, types).sum(1) - ref.sum(1)
    print('[grpo] change of each sample\'s log-probability, by advantage: ' + '  '.join(f'{x:+.2f}:{y:+.1f}' for x, y in zip(adv.tolist(), lp.tolist())))
    print(f'[grpo] reward of a fresh sample from the updated adapters: {sample(101)[2].mean().item():.4f}')
    print('[grpo] done: sampled ids trained as they were drawn - no decode / re-tokenize round trip')


if __name__ == '__main__':
    main()
