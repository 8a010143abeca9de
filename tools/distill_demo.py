"""The guidance-distillation loop closed once - a demonstration on the synthetic weights, not a result and not a test:

  teacher   a depth-2 ControlVAR samples a batch at cfg = 4 with distill_targets=True: the ids it drew and the guided logits
            softmax(sum_k coef_k logits_k) it drew every token from
  student   a copy of the teacher with LoRA adapters (cond_drop_rate = 0) takes a few Trainer.step_tokens(distill=targets.loss()) updates
            on that batch, the teacher's ids as its inputs and the guided distributions as its soft targets
  sample    the student then generates with cfg=None - one transformer row per sample, no guidance rows - beside the teacher's guided call

    python tools/distill_demo.py --depth 2 --batch 4 --iters 6

The KL printed per update is the step's loss, KL(teacher guided || student) averaged over the tokens; it falls on the batch it is trained on."""
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
    ap.add_argument('--lr', type=float, default=2e-3)
    ap.add_argument('--cfg', type=float, default=4.0)
    a = ap.parse_args()
    import torch
    from controlvar_amd import lora, models
    from controlvar_amd import train as T
    if not torch.cuda.is_available():
        raise SystemExit('distill_demo needs the GPU')
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
    sampling = dict(top_k=900, top_p=0.96)

    images_t, t = teacher.autoregressive_infer_cfg(B, cls, g_seed=seeds, cfg=a.cfg, cond_type=types, distill_targets=True, **sampling)
    print(f'[distill] teacher at cfg = {a.cfg}: {B} samples, targets logits {tuple(t.logits.shape)}, ids {tuple(t.ids_img.shape)} per half, '
          f'{int(t.sampled.sum())} of {t.sampled.numel()} tokens sampled')
    for u in range(a.iters):
        o = tr.step_tokens(t.ids_img, t.ids_ctrl, cls, types, distill=t.loss(), mask_first=t.mask_first)
        print(f'[distill] update {u}: KL(teacher guided || student) {o["loss"].item():.5f}  grad_norm {o["grad_norm"].item():.3f}')
    images_s = student.autoregressive_infer_cfg(B, cls, g_seed=seeds, cfg=None, cond_type=types, **sampling)
    images_u = teacher.autoregressive_infer_cfg(B, cls, g_seed=seeds, cfg=None, cond_type=types, **sampling)
    d = lambda x, y: (x.float() - y.float()).abs().mean().item()
    print(f'[distill] mean |pixel difference| to the teacher\'s guided sample: student at cfg=None {d(images_s, images_t):.4f}, '
          f'teacher at cfg=None (no distillation) {d(images_u, images_t):.4f}')
    print('[distill] done: the student generates with one row per sample; the teacher paid for two')


if __name__ == '__main__':
    main()
