"""Sparse guidance distillation closed once - a demonstration on the synthetic weights, not a result and not a test:

  teacher   a depth-2 ControlVAR samples a batch at cfg = 4 with distill_topn=N: the ids it drew and, per token, the N most likely codes of the
            guided distribution with their log-probabilities and the mass of the rest - N x 8 + 4 bytes per token, no (B, L, V) tensor
  student   a copy of the teacher with LoRA adapters (cond_drop_rate = 0) takes a few Trainer.step_tokens(distill=targets.loss()) updates

    python tools/topn_demo.py --depth 2 --batch 4 --iters 6 --topn 32

The KL printed is the step's loss before the first and after the last update: KL(teacher || student) over the N + 1 cells, averaged over the tokens."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--iters', type=int, default=6, help='distillation steps on the sampled batch')
    ap.add_argument('--topn', type=int, default=32)
    ap.add_argument('--lr', type=float, default=2e-3)
    ap.add_argument('--cfg', type=float, default=4.0)
    a = ap.parse_args()
    import torch
    from controlvar_amd import lora, models
    from controlvar_amd import train as T
    if not torch.cuda.is_available():
        raise SystemExit('topn_demo needs the GPU')
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    B = a.batch
    vae = models.build_vae(ch=32 if a.depth <= 4 else 160, compute_dtype=bf).to(dev)
    kw = dict(depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf, cond_drop_rate=0.0)
    teacher = models.build_control_var(vae, **kw).to(dev).eval()
    student = models.build_control_var(vae, **kw).to(dev).eval()
    student.load_state_dict(teacher.state_dict())
    lora.add_lora(student, r=16, dropout=0.0, seed=1)
    tr = T.Trainer(student, vae, peak_lr=a.lr, weight_decay=0.0, sche='lin0', warmup_it=0, max_it=1000, clip=2.0, drop_path=False, train_mode=False)
    g = torch.Generator().manual_seed(0)
    cls, types = torch.randint(0, 1000, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
    seeds = [100 + b for b in range(B)]
    _, t = teacher.autoregressive_infer_cfg(B, cls, g_seed=seeds, cfg=a.cfg, cond_type=types, distill_topn=a.topn, top_k=900, top_p=0.96)
    stored = sum(x.numel() * x.element_size() for x in (t.top_ids, t.top_logprobs, t.tail_logprob))
    dense = t.top_ids.shape[0] * t.top_ids.shape[1] * teacher.cfg.vocab * 4
    print(f'[topn] teacher at cfg = {a.cfg}: {B} samples, top_ids {tuple(t.top_ids.shape)}, {stored / B / 1e3:.0f} KB of targets per sample '
          f'({dense / stored:.0f} times less than the dense logits); mean listed mass {1 - t.tail_logprob.exp().mean().item():.4f}')
    kls = [tr.step_tokens(t.ids_img, t.ids_ctrl, cls, types, distill=t.loss(), mask_first=t.mask_first)['loss'].item() for _ in range(a.iters + 1)]
    print(f'[topn] KL(teacher guided || student) before the first update {kls[0]:.5f}, after {a.iters} updates {kls[-1]:.5f}')


if __name__ == '__main__':
    main()
