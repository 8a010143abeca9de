"""Per-request guidance, top-k, top-p and seed on the MI355X.  One invariant: in per-request mode, row b of a batch produces exactly what the
scalar call produces at B = 1 with (label_b, cond_type_b, cfg_b, top_k_b, top_p_b, g_seed = seed_b).  The scalar `ops.cfg_sample` - pinned
to the reference by the fixtures - is the oracle throughout, and every comparison is torch.equal: no tolerance anywhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import models, ops  # noqa: E402
from controlvar_amd._lib import CvarError  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, VarConfig  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
V = 4096
# five requests: sampled, greedy, sampled, sampled, sampled - the greedy row rides between sampled ones; one seed has its top bit set
TOP_K = [50, 1, 900, 0, 4096]
TOP_P = [0.5, 0.96, 0.96, 1.0, 0.0]
SEEDS = [11, 12, 2 ** 64 - 3, 0, 123456789012345]
GUIDE = [1.5, 4.0, 0.25, 3.0, 7.5]


def as_i64(seeds):
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64)


def row_coefs(B, nrep, stage, nstage=10):
    """distinct fp32 weights per row, the eager expressions of the 2- and the 4-branch form at `stage`"""
    ratio = stage / (nstage - 1)
    out = np.zeros((B, 4), dtype=np.float32)
    for b in range(B):
        t = GUIDE[b % 5] * ratio
        out[b, :nrep] = [1 + t, -t] if nrep == 2 else [1 + t, 0.5 * t - t, 0.25 * t - 0.5 * t, -0.25 * t]
    return torch.from_numpy(out)


def make_logits(B, nrep, l, ldv, seed, Vc=V):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(nrep * B, l, ldv, generator=g) * 3.0
    if ldv > Vc:
        lg[:, :, Vc:] = 100.0                          # columns behind the codes: larger than every logit, must never be read
    return lg


def rows_call(lg, B, nrep, l, Vc, n_draw, coef, top_k, top_p, seed, stage, ldv=0):
    dev = lg.device
    idx = torch.full((n_draw * B, l), -1, dtype=torch.int32, device=dev)
    comb = torch.full((B, l, Vc), float('nan'), device=dev)
    mg = torch.full((B, l), float('nan'), device=dev)
    kept = torch.full((B, l), -1, dtype=torch.int32, device=dev)
    ops.cfg_sample_rows(lg, B, nrep, l, Vc, coef, top_k, top_p, seed, stage, n_draw, idx, comb, mg, kept, ldv=ldv)
    return idx, comb, mg, kept


def scalar_call(lg_row, nrep, l, Vc, n_draw, coef, top_k, top_p, seed, stage, ldv=0):
    """the oracle: the scalar kernels at B = 1 on one row's logits (nrep, l, ldv)"""
    dev = lg_row.device
    idx = torch.full((n_draw, l), -1, dtype=torch.int32, device=dev)
    comb = torch.full((1, l, Vc), float('nan'), device=dev)
    mg = torch.full((1, l), float('nan'), device=dev)
    kept = torch.full((1, l), -1, dtype=torch.int32, device=dev)
    ops.cfg_sample(lg_row.contiguous(), 1, nrep, l, Vc, [float(c) for c in coef[:nrep]], int(top_k), float(top_p), int(seed), stage, n_draw, idx, comb, mg, kept, ldv=ldv)
    return idx, comb, mg, kept


def check_rows_against_scalar(dev, lg, B, nrep, l, Vc, n_draw, stage, ldv=0, rows=None, top_k=TOP_K, top_p=TOP_P, seeds=SEEDS):
    coef = row_coefs(B, nrep, stage)
    ks = [top_k[b % len(top_k)] for b in range(B)]
    ps = torch.tensor([top_p[b % len(top_p)] for b in range(B)], dtype=torch.float32)
    sd = [seeds[b % 5] + b // 5 for b in range(B)]
    got = rows_call(lg, B, nrep, l, Vc, n_draw, coef.to(dev), torch.tensor(ks, dtype=torch.int32, device=dev), ps.to(dev), as_i64(sd).to(dev), stage, ldv=ldv)
    idx, comb, mg, kept = got
    assert int(idx.min()) >= 0 and int(idx.max()) < Vc
    for b in (range(B) if rows is None else rows):
        lg_row = lg.view(nrep, B, l, -1)[:, b]
        ridx, rcomb, rmg, rkept = scalar_call(lg_row, nrep, l, Vc, n_draw, coef[b].tolist(), ks[b], float(ps[b]), sd[b], stage, ldv=ldv)
        assert torch.equal(idx.view(n_draw, B, l)[:, b], ridx), (b, stage)
        assert torch.equal(comb[b], rcomb[0]), (b, stage)
        assert torch.equal(mg[b], rmg[0]) and torch.equal(kept[b], rkept[0]), (b, stage)
        if ks[b] == 1:
            assert bool((kept[b] == 1).all()) and torch.equal(idx.view(n_draw, B, l)[:, b], idx.view(n_draw, B, l)[:1, b].expand(n_draw, l))
    return got


# ------------------------------------------------------------------------------------------------------------- 1. rows against the scalar kernel
@pytest.mark.parametrize('nrep,n_draw', [(2, 1), (4, 4)])
@pytest.mark.parametrize('l', [1, 4])
def test_every_row_equals_the_scalar_kernel_at_batch_one(gpu_device, l, nrep, n_draw):
    B = 5
    lg = make_logits(B, nrep, l, V, seed=100 + 10 * l + nrep).to(gpu_device)
    for stage in (0, 7):
        check_rows_against_scalar(gpu_device, lg, B, nrep, l, V, n_draw, stage)


def test_a_head_wider_than_the_codebook(gpu_device):
    """V = 4000 codes in rows of ldv = 4096 floats: the 96 columns behind the codes hold the largest values and are never read"""
    B, l, Vc = 5, 4, 4000
    lg = make_logits(B, 2, l, 4096, seed=7, Vc=Vc).to(gpu_device)
    idx, comb, _, kept = check_rows_against_scalar(gpu_device, lg, B, 2, l, Vc, 1, 3, ldv=4096)
    assert float(comb.max()) < 100.0 and int(kept.max()) <= Vc


def test_duplicated_maxima_in_a_greedy_row_lowest_index_wins(gpu_device):
    B, l = 5, 4
    lg = make_logits(B, 2, l, V, seed=8)
    pair = lg.view(2, B, l, V)
    for e in (3000, 77, 1234):                          # row 1 is the greedy one: three exactly tied maxima of the combined logits
        pair[0, 1, :, e] = 50.0
        pair[1, 1, :, e] = -2.0
    pair[0, 2, :, 5] = pair[0, 2, :, 9] = 40.0          # and a tie at the top of a sampled row: both kept, drawn among as the scalar kernel does
    pair[1, 2, :, 5] = pair[1, 2, :, 9] = 0.0
    idx, _, mg, kept = check_rows_against_scalar(gpu_device, lg.to(gpu_device), B, 2, l, V, 1, 5)
    assert idx[1].tolist() == [77] * l and mg[1].tolist() == [0.0] * l and kept[1].tolist() == [1] * l


# ------------------------------------------------------------------------------------------------------------- 2. slot independence
def test_a_request_does_not_depend_on_its_slot_or_its_neighbours(gpu_device):
    dev = gpu_device
    B, nrep, n_draw, l, stage = 5, 4, 4, 16, 4
    lg = make_logits(B, nrep, l, V, seed=21)
    lg.view(nrep, B, l, V)[:, 3] = lg.view(nrep, B, l, V)[:, 0]                  # rows 0 and 3: the same request twice
    coef = row_coefs(B, nrep, stage)
    coef[3] = coef[0]
    ks = torch.tensor([0, 1, 900, 0, 50], dtype=torch.int32)
    ps = torch.tensor([0.96, 0.0, 0.5, 0.96, 1.0])
    sd = as_i64([5, 6, 7, 5, 2 ** 63 + 9])

    def call(lgs, c, k, p, s):
        return rows_call(lgs.contiguous().to(dev), B, nrep, l, V, n_draw, c.contiguous().to(dev), k.to(dev), p.to(dev), s.to(dev), stage)
    idx, comb, mg, kept = call(lg, coef, ks, ps, sd)
    assert torch.equal(idx.view(n_draw, B, l)[:, 0], idx.view(n_draw, B, l)[:, 3]) and torch.equal(kept[0], kept[3])
    perm = torch.tensor([2, 4, 0, 3, 1])
    pidx, pcomb, pmg, pkept = call(lg.view(nrep, B, l, V)[:, perm].reshape(nrep * B, l, V), coef[perm], ks[perm], ps[perm], sd[perm])
    assert torch.equal(pidx.view(n_draw, B, l), idx.view(n_draw, B, l)[:, perm.to(dev)])
    assert torch.equal(pcomb, comb[perm.to(dev)]) and torch.equal(pmg, mg[perm.to(dev)]) and torch.equal(pkept, kept[perm.to(dev)])
    other = sd.clone()
    other[0], other[1] = 1005, 1006                     # another seed for one sampled and for the greedy request
    oidx = call(lg, coef, ks, ps, other)[0].view(n_draw, B, l)
    assert not torch.equal(oidx[:, 0], idx.view(n_draw, B, l)[:, 0])
    assert torch.equal(oidx[:, 1:], idx.view(n_draw, B, l)[:, 1:])               # the greedy row and every row whose seed stayed


# ------------------------------------------------------------------------------------------------------------- 3. offsets
def test_rows_kernel_at_the_headline_logits(gpu_device):
    """one launch on logits [2 x 512][256][4096] fp32 (2^30 elements, 4.3 GB: rows past 2^32 bytes); rows 0, 255, 256 and 511 against the
    scalar kernel at B = 1.  Peak: logits 4.3 GB + combined 2.1 GB."""
    dev = gpu_device
    free, _ = torch.cuda.mem_get_info(dev)
    if free < (10 << 30):
        pytest.skip(f'needs 10 GB of free device memory, {free} bytes available')
    B, l = 512, 256
    g = torch.Generator(device=dev).manual_seed(31)
    lg = torch.empty(2 * B, l, V, device=dev)
    flat = lg.view(-1)
    for lo in range(0, flat.numel(), 1 << 28):
        flat[lo:lo + (1 << 28)].normal_(0.0, 3.0, generator=g)
    ks, ps = [TOP_K[b % 5] for b in range(B)], [TOP_P[b % 5] for b in range(B)]
    for b, k, p in ((0, 900, 0.96), (255, 1, 0.0), (256, 0, 0.5), (511, 50, 1.0)):          # the compared rows: sampled, greedy, sampled, sampled
        ks[b], ps[b] = k, p
    check_rows_against_scalar(dev, lg, B, 2, l, V, 1, 6, rows=(0, 255, 256, 511), top_k=ks, top_p=ps)


# ------------------------------------------------------------------------------------------------------------- 4. argument edges
def test_null_tables_noise_and_soft_output_are_refused_and_nothing_is_launched(gpu_device):
    dev = gpu_device
    B, l = 2, 3
    lg = make_logits(B, 2, l, V, seed=41).to(dev)
    good = dict(coef=row_coefs(B, 2, 1).to(dev), top_k=torch.tensor([0, 1], dtype=torch.int32, device=dev), top_p=torch.zeros(B, device=dev),
                seed=torch.zeros(B, dtype=torch.int64, device=dev))
    idx = torch.full((B, l), -1, dtype=torch.int32, device=dev)

    def call(nrep=2, n_draw=1, Vc=V, ldv=0, **kw):
        a = {**good, **kw}
        extra = {k: a.pop(k) for k in ('expo', 'soft_out') if k in a}
        ops.cfg_sample_rows(lg, B, nrep, l, Vc, a['coef'], a['top_k'], a['top_p'], a['seed'], 0, n_draw, idx, ldv=ldv, **extra)
    for name in good:
        with pytest.raises(CvarError, match='invalid'):
            call(**{name: None})
    with pytest.raises(CvarError, match='unsupported'):
        call(expo=torch.ones(B, l, V, device=dev))
    with pytest.raises(CvarError, match='unsupported'):
        call(soft_out=torch.zeros(B, l, 32, device=dev))
    for bad in (dict(nrep=5), dict(nrep=0), dict(n_draw=5), dict(Vc=V + 1)):
        with pytest.raises(CvarError, match='unsupported'):
            call(**bad)
    with pytest.raises(CvarError, match='invalid'):
        call(ldv=V - 1)
    for name, wrong in (('coef', good['coef'][:, :2]), ('coef', good['coef'].double()), ('top_k', good['top_k'].long()), ('top_p', good['top_p'].cpu()),
                        ('seed', good['seed'][:1]), ('seed', good['seed'].int())):
        with pytest.raises(ValueError, match=name):
            call(**{name: wrong})
    torch.cuda.synchronize()
    assert bool((idx == -1).all())                      # no refused call launched anything
    call()
    assert int(idx.min()) >= 0


# ------------------------------------------------------------------------------------------------------------- 5. - 7. end to end
def make(dtype, dev):
    """the depth-3, C = 256, ch = 32 models of tests/test_gpu_cond_graph.py"""
    cfg = VarConfig(depth=3, embed_dim=256, num_heads=4)
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    m = models.ControlVAR(vae, depth=cfg.depth, embed_dim=cfg.C, num_heads=cfg.H, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=dtype,
                          cond_drop_rate=0.0).to(dev).eval()
    return vae, m


@pytest.fixture(scope='module')
def bf16_models(gpu_device):
    return make(BF16, gpu_device)


def traced(m, n_draw):
    tr = m.last_trace
    B = tr['logits'][0].shape[0]
    return ([x.view(n_draw, B, -1).clone() for x in tr['idx']], [x.clone() for x in tr['logits']], [x.clone() for x in tr['margin']])


def assert_row_equals_single(batch, b, single, img, img1, what):
    for si, (x, y) in enumerate(zip(batch[1], single[1])):
        assert torch.equal(x[b], y[0]), (what, 'combined logits', b, si, float((x[b] - y[0]).abs().max()))
    for si, (x, y) in enumerate(zip(batch[2], single[2])):
        assert torch.equal(x[b], y[0]), (what, 'margin', b, si)
    for si, (x, y) in enumerate(zip(batch[0], single[0])):
        assert torch.equal(x[:, b], y[:, 0]), (what, 'ids', b, si)
    assert torch.equal(img[b], img1[0]), (what, 'image', b)


def test_a_mixed_batch_equals_its_batch_one_calls(gpu_device, bf16_models):
    """under deterministic_plan=True row b of a per-request batch is the scalar call at B = 1 with row b's scalars: traced ids, per-scale
    combined logits, margins and the image, bit for bit - joint generation at B = 4 (one request greedy), then conditional generation at
    B = 3 with teacher-forced control ids and one triple of guidance scales per row"""
    vae, m = bf16_models
    m.deterministic_plan = True
    try:
        B = 4
        labels, types = torch.tensor([1, 500, 999, 7]), torch.tensor([0, 3, 1, 2])
        cfgs, ks, ps, seeds = [1.5, 4.0, 3.0, 0.5], [900, 1, 0, 50], [0.96, 0.0, 0.5, 1.0], [11, 12, 2 ** 64 - 5, 14]
        img = m.autoregressive_infer_cfg(B, labels, g_seed=seeds, cfg=cfgs, top_k=ks, top_p=ps, cond_type=types, _trace=True)
        batch = traced(m, 1)
        for b in range(B):
            img1 = m.autoregressive_infer_cfg(1, labels[b:b + 1], g_seed=seeds[b], cfg=cfgs[b], top_k=ks[b], top_p=ps[b], cond_type=types[b:b + 1], _trace=True)
            assert_row_equals_single(batch, b, traced(m, 1), img, img1, 'joint')
        B = 3
        labels, types = torch.tensor([3, 2, 1]), torch.tensor([2, 0, 1])
        ids = vae.img_to_idxBl(synth_images(B, 256, seed=31).to(gpu_device))
        triples = np.array([(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (4.0, 0.5, 2.5)])
        ks, ps, seeds = [1, 900, 0], [0.0, 0.96, 0.9], [21, 22, 23]
        img = m.conditional_infer_cfg(B, labels, g_seed=seeds, cfg=triples, top_k=ks, top_p=ps, cond_type=types, c_mask=ids, _trace=True)
        batch = traced(m, 4)
        for b in range(B):
            img1 = m.conditional_infer_cfg(1, labels[b:b + 1], g_seed=seeds[b], cfg=tuple(triples[b].tolist()), top_k=ks[b], top_p=ps[b], cond_type=types[b:b + 1],
                                           c_mask=[i[b:b + 1] for i in ids], _trace=True)
            assert_row_equals_single(batch, b, traced(m, 4), img, img1, 'conditional')
    finally:
        m.deterministic_plan = False


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_all_greedy_uniform_guidance_equals_the_scalar_call(gpu_device, bf16_models, dtype):
    """the bridge to the pinned path: per-request mode with every row greedy and one guidance scale is the scalar call at the same B - ids,
    combined logits and images, under the default plan"""
    vae, m = bf16_models if dtype == BF16 else make(F32, gpu_device)
    B = 3
    labels, types = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2])
    want = m.autoregressive_infer_cfg(B, labels, g_seed=5, cfg=3.0, top_k=1, cond_type=types, _trace=True)
    ref = traced(m, 1)
    got = m.autoregressive_infer_cfg(B, labels, g_seed=[5, 6, 7], cfg=[3.0] * B, top_k=[1] * B, cond_type=types, _trace=True)
    rows = traced(m, 1)
    for part in range(3):
        for si, (x, y) in enumerate(zip(rows[part], ref[part])):
            assert torch.equal(x, y), (part, si)
    assert torch.equal(got, want)


PARAMS = (dict(g_seed=[1, 2, 3], cfg=[1.5, 3.0, 4.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5]),
          dict(g_seed=[7, 7, 2 ** 64 - 1], cfg=2.0, top_k=[1, 50, 900], top_p=0.9))


def check_graph(run, eager, wrong_length, too_large):
    outs = []
    for p in PARAMS:
        a = run(**p)
        assert torch.equal(a, eager(**p))
        outs.append(a)
    assert not torch.equal(outs[0], outs[1])
    reseeded = dict(PARAMS[1], g_seed=[8, 9, 10])
    c = run(**reseeded)
    assert not torch.equal(c, outs[1]) and torch.equal(c, eager(**reseeded))
    again = run(**PARAMS[1])
    assert torch.equal(again, outs[1])
    # a refused call leaves the buffers of the graph as they were
    with pytest.raises(ValueError, match='one per batch row'):
        run(**wrong_length)
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        run(**too_large)
    with pytest.raises(ValueError, match='must be given per row'):
        run(**dict(PARAMS[0], label_B=None))
    assert torch.equal(run(**PARAMS[1]), again)


def test_one_joint_graph_serves_every_parameter_set(gpu_device, bf16_models):
    vae, m = bf16_models
    B = 3
    labels, types = torch.tensor([7, 500, 999]), torch.tensor([3, 3, 0])
    graph = m.graphed_generator(B, cfg=2.5, top_k=600, top_p=0.8, per_request=True)

    def run(label_B=labels, **p):
        return graph(label_B, types, **p)

    def eager(**p):
        return m.autoregressive_infer_cfg(B, labels, cond_type=types, **p)
    check_graph(run, eager, dict(PARAMS[0], top_k=[1, 2]), dict(PARAMS[0], top_k=[1, V + 1, 0]))
    # what was given at capture are the defaults of run
    assert torch.equal(run(g_seed=[4, 5, 6]), eager(g_seed=[4, 5, 6], cfg=2.5, top_k=600, top_p=0.8))
    # today's form refuses the per-request keywords in words
    scalar = m.graphed_generator(B, cfg=2.5, top_k=600, top_p=0.8)
    with pytest.raises(TypeError, match='per_request=False'):
        scalar(labels, types, g_seed=1, top_k=1)


def test_one_conditional_graph_serves_every_parameter_set(gpu_device, bf16_models):
    vae, m = bf16_models
    B = 3
    labels, types = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2])
    ids = vae.img_to_idxBl(synth_images(B, 256, seed=32).to(gpu_device))
    graph = m.graphed_conditional_generator(B, given='control', source='ids', per_request=True)
    triples = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (4.0, 0.5, 2.5)]

    def guidance(p):
        return dict(p, cfg=triples if isinstance(p['cfg'], list) else (p['cfg'], 1.0, 0.5))

    def run(label_B=labels, **p):
        return graph(label_B, types, ids, **guidance(p))

    def eager(**p):
        return m.conditional_infer_cfg(B, labels, cond_type=types, c_mask=ids, **guidance(p))
    check_graph(run, eager, dict(PARAMS[0], top_k=[1, 2]), dict(PARAMS[0], top_k=[1, V + 1, 0]))
    assert torch.equal(graph.ids().long(), torch.cat(ids, dim=1))
