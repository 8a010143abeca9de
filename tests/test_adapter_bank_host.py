"""The adapter bank on the host (controlvar_amd/lora.py attach_adapters / pack_bank): packing for 1, 3 and 8 adapters of mixed
ranks in both compute dtypes, the adaLN block-diagonal against a dense einsum, every layout load_lora reads, every refusal (each raised
before any device work, so a CPU model shows it), and the expansion of request ids to sequence slots."""
import numpy as np
import pytest
import torch

from controlvar_amd import lora, models
from controlvar_amd.models import _RequestTable, _request_table
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN

F32, BF16 = torch.float32, torch.bfloat16
C, DEPTH, HID = 128, 2, 512
RANKS = (16, 5, 1)


def make(shared_aln=False, control=True):
    vae = models.build_vae(ch=32, compute_dtype=F32)
    if control:
        return models.ControlVAR(vae, depth=DEPTH, embed_dim=C, num_heads=2, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=F32,
                                 cond_drop_rate=0.0, shared_aln=shared_aln)
    return models.VAR(vae, depth=DEPTH, embed_dim=C, num_heads=2, patch_nums=PN, compute_dtype=F32, cond_drop_rate=0.0)


@pytest.fixture(scope='module')
def model():
    return make()


def adapter_state(m, r, seed, layout='own', module=False, b_std=0.2):
    """a random adapter of rank r for m's targets in one of the layouts load_lora reads"""
    g = torch.Generator().manual_seed(seed)
    mods = dict(m.named_modules())
    own = {}
    for t in lora.target_names(m):
        out_f, in_f = mods[t]._parameters['weight'].shape
        own[f'{t}.lora_A.default.weight'] = torch.randn(r, in_f, generator=g) / in_f ** 0.5
        own[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * b_std
    if layout == 'own':
        sd = own
    elif layout == 'adapter':                             # peft's adapter file: no adapter name, everything under base_model.model.
        sd = {lora.PEFT_PREFIX + k.replace('.default.', '.'): v for k, v in own.items()}
    elif layout == 'peft':                                # peft's whole model: base weights under .base_layer.
        sd = {}
        targets = lora.target_names(m)
        for k, v in m.state_dict().items():
            t = next((t for t in targets if k.startswith(t + '.')), None)
            sd[lora.PEFT_PREFIX + (t + '.base_layer' + k[len(t):] if t else k)] = v
        sd.update({lora.PEFT_PREFIX + k: v for k, v in own.items()})
    else:
        raise ValueError(layout)
    if module:
        sd = {'module.' + k: v for k, v in sd.items()}
    return sd, own


def base_pack(m, dtype):
    sd = m.state_dict()
    blk = lambda s: torch.stack([sd[f'blocks.{i}.{s}'] for i in range(DEPTH)]).to(dtype)
    return {'w_proj': blk('attn.proj.weight'), 'w_fc1': blk('ffn.fc1.weight'), 'w_fc2': blk('ffn.fc2.weight'),
            'w_ada': torch.cat([sd[f'blocks.{i}.ada_lin.1.weight'] for i in range(DEPTH)] + [sd['head_nm.ada_lin.1.weight']]).to(dtype)}


def attach(m, n, alpha=32):
    owns = []
    srcs = []
    for k in range(n):
        sd, own = adapter_state(m, RANKS[k % 3], 100 + k, layout=('own', 'adapter', 'peft')[k % 3], module=k % 2 == 1)
        srcs.append(sd)
        owns.append(own)
    lora.attach_adapters(m, srcs, alpha=alpha)
    return owns


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('n', [1, 3, 8])
def test_packing(model, n, dtype):
    m = model
    keys = list(m.state_dict())
    owns = attach(m, n)
    try:
        assert list(m.state_dict()) == keys and lora.has_adapters(m) and not lora.has_lora(m)       # a bank is no set of parameters
        bank = m._adapter_bank
        assert bank['ranks'] == [RANKS[k % 3] for k in range(n)] and bank['scales'] == [32 / r for r in bank['ranks']]
        P = base_pack(m, dtype)
        BK = lora.pack_bank(bank, P, C, DEPTH, dtype)
        es = 2 if dtype == BF16 else 4
        assert (BK['kx'] * es) % 128 == 0 and (BK['kxa'] * es) % 128 == 0 and BK['kx'] >= 16 * n and BK['kxa'] >= 16 * n * (DEPTH + 1)
        assert BK['kx'] - 16 * n < 128 // es and BK['kx'] == lora.bank_kx(n, dtype)
        assert torch.equal(BK['scale'], torch.tensor(bank['scales']))
        for kind, name in lora.BANK_KINDS:
            A, W = BK['A'][kind], BK['W'][kind]
            n_out, k_in = P['w_' + kind].shape[1:]
            assert A.shape == (DEPTH, n, 16, k_in) and W.shape == (DEPTH, n_out, k_in + BK['kx']) and A.dtype == W.dtype == dtype
            assert torch.equal(W[:, :, :k_in], P['w_' + kind])
            assert not W[:, :, k_in + 16 * n:].any()
            for k in range(n):
                r = bank['ranks'][k]
                for i in range(DEPTH):
                    assert torch.equal(A[i, k, :r], owns[k][f'blocks.{i}.{name}.lora_A.default.weight'].to(dtype))
                    assert torch.equal(W[i, :, k_in + 16 * k:k_in + 16 * k + r], owns[k][f'blocks.{i}.{name}.lora_B.default.weight'].to(dtype))
                assert not A[:, k, r:].any() and not W[:, :, k_in + 16 * k + r:k_in + 16 * k + 16].any()
    finally:
        lora.detach_adapters(m)
    assert not lora.has_adapters(m)


@pytest.mark.parametrize('n', [1, 3, 8])
def test_adaln_block_diagonal_against_a_dense_einsum(model, n):
    m = model
    owns = attach(m, n, alpha=[32 + k for k in range(n)])
    try:
        bank = m._adapter_bank
        assert bank['scales'] == [(32 + k) / RANKS[k % 3] for k in range(n)]
        P = base_pack(m, F32)
        BK = lora.pack_bank(bank, P, C, DEPTH, F32)
        n_ada = P['w_ada'].shape[0]
        assert BK['W']['ada'].shape == (n_ada, C + BK['kxa']) and BK['A']['ada'].shape == (DEPTH + 1, n, 16, C)
        g = torch.Generator().manual_seed(3)
        R = 2 * n + 1
        cs = torch.randn(R, C, generator=g).double()
        slot = [-1] + [k for k in range(n)] * 2
        # the operand the kernels build: [cs | one 16-column group per (target, slot): s x A^T in the row's slot, zeros elsewhere]
        csa = torch.zeros(R, C + BK['kxa'], dtype=torch.float64)
        csa[:, :C] = cs
        for b, k in enumerate(slot):
            for t in range(DEPTH + 1):
                if k >= 0:
                    c0 = C + 16 * (t * n + k)
                    csa[b, c0:c0 + 16] = bank['scales'][k] * cs[b] @ BK['A']['ada'][t, k].double().t()
        got = csa @ BK['W']['ada'].double().t()
        names = [f'blocks.{t}.ada_lin.1' for t in range(DEPTH)] + ['head_nm.ada_lin.1']
        want = cs @ P['w_ada'].double().t()
        for b, k in enumerate(slot):
            if k < 0:
                continue
            for t, name in enumerate(names):
                A = owns[k][name + '.lora_A.default.weight'].double()
                Bm = owns[k][name + '.lora_B.default.weight'].double()
                want[b, t * 6 * C:t * 6 * C + Bm.shape[0]] += bank['scales'][k] * torch.einsum('c,rc,or->o', cs[b], A, Bm)
        assert (got - want).abs().max() < 1e-9 * want.abs().max()
    finally:
        lora.detach_adapters(m)


def test_merged_adapter_state_is_w_plus_s_b_a(model):
    m = model
    owns = attach(m, 3)
    try:
        sd = m.state_dict()
        out = lora.merged_adapter_state(sd, m._adapter_bank, 1)
        assert set(out) == set(sd)
        t = 'blocks.1.ffn.fc2'
        want = sd[t + '.weight'] + (32 / 5) * owns[1][t + '.lora_B.default.weight'] @ owns[1][t + '.lora_A.default.weight']
        assert torch.allclose(out[t + '.weight'], want, atol=1e-6) and torch.equal(out['blocks.0.attn.mat_qkv.weight'], sd['blocks.0.attn.mat_qkv.weight'])
    finally:
        lora.detach_adapters(m)


def test_refusals(model):
    m = model
    good, _ = adapter_state(m, 4, 1)
    missing = dict(good)
    del missing['blocks.0.attn.proj.lora_A.default.weight']
    extra = dict(good, **{'blocks.0.attn.mat_qkv.lora_A.default.weight': torch.zeros(4, C)})
    for bad in (missing, extra):
        with pytest.raises(KeyError, match='adapter state'):
            lora.attach_adapters(m, [good, bad])
    wrong = dict(good)
    wrong['blocks.1.ffn.fc1.lora_B.default.weight'] = torch.zeros(HID, 5)
    with pytest.raises(ValueError, match=r'blocks\.1\.ffn\.fc1\.lora_B\.default\.weight: shape'):
        lora.attach_adapters(m, [wrong])
    with pytest.raises(NotImplementedError, match='rank 17'):
        lora.attach_adapters(m, [adapter_state(m, 17, 2)[0]])
    with pytest.raises(NotImplementedError, match='9 adapters'):
        lora.attach_adapters(m, [good] * 9)
    with pytest.raises(NotImplementedError, match='0 adapters'):
        lora.attach_adapters(m, [])
    with pytest.raises(ValueError, match='alpha'):
        lora.attach_adapters(m, [good, good], alpha=[32])
    assert not lora.has_adapters(m)                      # nothing half-attached
    with pytest.raises(RuntimeError, match='no adapter bank'):
        lora.detach_adapters(m)
    with pytest.raises(NotImplementedError, match='shared_aln'):
        lora.attach_adapters(make(shared_aln=True), [good])
    # a bank and add_lora exclude each other, in words
    with_lora = make()
    lora.add_lora(with_lora, r=4)
    with pytest.raises(RuntimeError, match='mutually exclusive'):
        lora.attach_adapters(with_lora, [good])
    lora.attach_adapters(m, [good])
    try:
        with pytest.raises(RuntimeError, match='mutually exclusive'):
            lora.add_lora(m, r=4)
    finally:
        lora.detach_adapters(m)


def test_adapter_ids(model):
    assert lora.adapter_ids(2, 3, 3).tolist() == [2, 2, 2] and lora.adapter_ids(-1, 2, 1).tolist() == [-1, -1]
    assert lora.adapter_ids([0, -1, 2], 3, 3).dtype == np.int32
    assert lora.adapter_ids(torch.tensor([1, 0]), 2, 2).tolist() == [1, 0] and lora.adapter_ids(np.array([0, 0], dtype=np.int64), 2, 1).tolist() == [0, 0]
    for bad in ([0, 3, 1], [0, -2, 1], 3):
        with pytest.raises(ValueError, match='id out of range'):
            lora.adapter_ids(bad, 3, 3)
    for bad in ([0, 1], [[0, 1, 2]], torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(ValueError, match='one per batch row'):
            lora.adapter_ids(bad, 3, 3)
    for bad in ([0.0, 1.0, 2.0], ['a', 'b', 'c']):
        with pytest.raises(ValueError, match='integers expected'):
            lora.adapter_ids(bad, 3, 3)


def test_generation_refuses_on_the_host_before_any_device_work(model):
    """the model lives on the CPU: whatever reaches the device path raises 'GPU only', so these refusals came first"""
    m = model
    labels, types = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2])
    with pytest.raises(RuntimeError, match='no bank attached'):
        m.autoregressive_infer_cfg(3, labels, cond_type=types, adapter=[0, 0, 0])
    with pytest.raises(RuntimeError, match='no bank attached'):
        m.edit_infer_cfg(3, labels, types, adapter=0)
    with pytest.raises(RuntimeError, match='no bank attached'):
        m.graphed_generator(3, per_request=True, adapters=True)
    attach(m, 3)
    try:
        for call in (lambda **k: m.autoregressive_infer_cfg(3, labels, cond_type=types, **k), lambda **k: m.conditional_infer_cfg(3, labels, cond_type=types, **k),
                     lambda **k: m.edit_infer_cfg(3, labels, types, **k)):
            with pytest.raises(ValueError, match='id out of range'):
                call(adapter=[0, 3, 1])
            with pytest.raises(ValueError, match='one per batch row'):
                call(adapter=[0, 1])
            # the refusals of per-request mode apply in the same words
            with pytest.raises(NotImplementedError, match='more_smooth is not offered'):
                call(adapter=0, more_smooth=True)
        with pytest.raises(ValueError, match='must be given per row'):
            m.autoregressive_infer_cfg(3, None, cond_type=types, adapter=0)
        m.sampler = 'torch'
        try:
            with pytest.raises(NotImplementedError, match="sampler='torch' is not offered"):
                m.autoregressive_infer_cfg(3, labels, cond_type=types, adapter=0)
        finally:
            m.sampler = 'counter'
        with pytest.raises(ValueError, match='per_request=True'):
            m.graphed_generator(3, adapters=True)
        with pytest.raises(RuntimeError, match='GPU only'):                 # a valid call gets past every host check
            m.autoregressive_infer_cfg(3, labels, cond_type=types, adapter=[0, -1, 2])
    finally:
        lora.detach_adapters(m)
    v = make(control=False)
    with pytest.raises(RuntimeError, match='no bank attached'):
        v.autoregressive_infer_cfg(2, torch.tensor([1, 2]), adapter=[0, 0])
    with pytest.raises(RuntimeError, match='no bank attached'):
        v.edit_infer_cfg(2, torch.tensor([1, 2]), adapter=[0, 0])


@pytest.mark.parametrize('nrep', [2, 4])
def test_request_ids_expand_to_sequence_slots(nrep):
    """the CFG rows are branch-major (row = branch * B + b, as _prepare_rows lays out labels): every branch of request b carries its id"""
    B, nstage = 5, 10
    ids = lora.adapter_ids([0, -1, 2, 1, 0], B, 3)
    slots = lora.sequence_slots(ids, nrep)
    assert slots.dtype == np.int32 and slots.shape == (nrep * B,)
    for rep in range(nrep):
        for b in range(B):
            assert slots[rep * B + b] == ids[b]
    # ... and ride behind the request table in the same host buffer: one upload
    four = nrep == 4
    cfg = (1.5, 1.0, 0.5) if four else 1.5
    tab = _request_table(B, cfg, 0, 0.0, [1, 2, 3, 4, 5], four, 4096, nstage, slots=slots)
    plain = _request_table(B, cfg, 0, 0.0, [1, 2, 3, 4, 5], four, 4096, nstage)
    assert plain.slot is None and plain.host.numel() == _RequestTable.nbytes(B, nstage)
    assert tab.host.numel() == _RequestTable.nbytes(B, nstage) + 4 * nrep * B
    assert torch.equal(tab.host[:plain.host.numel()], plain.host)
    copy = tab.host.clone()
    assert tab.slot_view(copy).tolist() == slots.tolist()
    assert all(torch.equal(a, b) for a, b in zip(tab.views(copy), plain.views(plain.host)))
