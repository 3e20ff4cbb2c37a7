"""GPU parity of the fused clip + optimiser kernels (csrc/optim.hip) -- the kernels every bench workload runs each step.

* three full train iterations (forward, joint loss, backward, clip, update) on the g3 goldens against the weights the
  imported reference holds after three torch.optim steps (`w_after.*`): Adadelta for loc_ctc / vgg_loc_ctc (the optimiser
  of config/libri_example.yaml and of every c2-c6 bench workload), Adam for dot_att / ctc_only.
  f32 mode: atol 3e-5 on every weight, loss of each iteration rel 3e-5.  bf16 mode: the first updates of both optimisers
  are sign-driven and step-sized whatever the gradient's magnitude (Adam +-lr = 1e-3 per step, Adadelta ~3e-4), so a
  near-zero gradient whose sign differs in bf16 moves a weight by up to 2 x 3 steps x that size: atol 6.5e-3 (Adam) /
  2e-3 (Adadelta) on single weights, and the mean |difference| must stay below 1e-4.
* clip active (||g|| > 5, reference solver.py:178), against the oracle's explicit clip_grad_norm_ / Adadelta / Adam formulas;
* the NaN guard of solver.py:179-182 decided on the device: a NaN gradient, and a whole step on a CTC-infeasible batch
  (inf loss -> NaN gradient), leave parameters, moments and the step counter untouched."""
import importlib
import os
import sys
import types
import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from golden_npz import load as load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def las():
    importlib.import_module('end-to-end-asr-pytorch_amd')
    return (importlib.import_module('end-to-end-asr-pytorch_amd.ops'), importlib.import_module('end-to-end-asr-pytorch_amd.asr'),
            importlib.import_module('end-to-end-asr-pytorch_amd.optim'))


def one_iteration(ops, model, opt, x, y, w):
    lens = ops.infer_lengths(x)
    ntok = ops.count_nonzero(y)
    ans_len = int(ntok.max().item())
    ctc_pred, _, att_pred, _ = model(x, ans_len, tf_rate=1.0, teacher=y, state_len=lens.cpu().tolist())
    loss, _, _ = ops.joint_loss(att_pred, ctc_pred, y, ntok, model.last_enc_len_dev, ans_len, w)
    loss.backward()
    opt.step(zero_grad=True)
    return float(loss.detach())


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['loc_ctc', 'vgg_loc_ctc', 'ctc_only', 'dot_att'])
def test_three_optimizer_steps_vs_reference(las, name, prec):
    ops, asr, optim = las
    from gen_golden import TINY
    d = load_golden(f'g3_step_{name}.npz')
    cfg = TINY[name]
    x = torch.tensor(d['x'], device=DEV)
    y = torch.tensor(d['y'], device=DEV)
    ops.set_precision(prec)
    try:
        model = asr.Seq2Seq(x, int(d['V']), cfg, device=DEV)
        model.load_reference_state({k[2:]: d[k] for k in d.files if k.startswith('w.')})
        o = cfg['optimizer']
        opt = optim.FlatOptimizer(model, o['type'], o['learning_rate'], eps=1e-8)
        opt.zero_grad()
        losses = [one_iteration(ops, model, opt, x, y, o['joint_ctc']) for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        ops.set_precision('bf16')
    assert int(model.status.item()) == 0
    assert int(opt.step_dev.item()) == 3 and float(opt.norm3[2]) == 0.0
    want = [float(d[f'loss_it{i}']) for i in range(3)]
    np.testing.assert_allclose(losses, want, rtol=3e-5 if prec == 'f32' else 2e-2)
    diffs = []
    for n, p in model.named_parameters():
        got, ref = p.detach().cpu().numpy(), d['w_after.' + n]
        np.testing.assert_allclose(got, ref, atol=3e-5 if prec == 'f32' else (6.5e-3 if o['type'] == 'Adam' else 2e-3), rtol=0,
                                   err_msg=n)
        diffs.append(np.abs(got - ref).ravel())
    if prec == 'bf16':
        assert float(np.concatenate(diffs).mean()) < 1e-4


def flat_holder(n, seed):
    g = torch.Generator().manual_seed(seed)
    m = types.SimpleNamespace()
    m.flat_params = torch.randn(n, generator=g).to(DEV)
    m.flat_grads = torch.zeros(n, device=DEV)
    return m, g


@pytest.mark.parametrize('opt_type,lr', [('Adadelta', 1.0), ('Adam', 1e-3)])
@pytest.mark.parametrize('world', [1, 4])
def test_clip_active_vs_oracle(las, opt_type, lr, world):
    """||g|| = 37 > GRAD_CLIP: coefficient 5/(37+1e-6) applied inside the update kernels, three steps (the moments of
    step k feed step k+1); world > 1: the all-reduced SUM is scaled by 1/world before the norm (dist.py)."""
    ops, asr, optim = las
    from oracle import las_ref as R
    n = 100_003                                     # not a multiple of 4: scalar tail of the norm kernel
    m, gen = flat_holder(n, 3)
    opt = optim.FlatOptimizer(m, opt_type, lr, eps=1e-8, world_size=world)
    p_ref = m.flat_params.cpu().clone()
    st = dict(m=torch.zeros(n), v=torch.zeros(n)) if opt_type == 'Adam' else dict(sq=torch.zeros(n), acc=torch.zeros(n))
    for k in range(3):
        g = torch.randn(n, generator=gen)
        g *= 37.0 / g.norm()
        m.flat_grads.copy_((g * world).to(DEV))     # what the sum all-reduce leaves in the buffer
        opt.step(zero_grad=True)
        gc = g.clone()
        total = R.clip_grad_norm([gc])
        p_ref = R.adam_update(p_ref, gc, st, lr, k + 1) if opt_type == 'Adam' else R.adadelta_update(p_ref, gc, st, lr)
        torch.cuda.synchronize()
        n3 = opt.norm3.cpu().tolist()
        assert abs(n3[0] - total) < 1e-3 and abs(n3[0] - 37.0) < 1e-3
        assert abs(n3[1] * world - 5.0 / (37.0 + 1e-6)) < 1e-6 and n3[2] == 0.0
        assert float(m.flat_grads.abs().max()) == 0.0
        np.testing.assert_allclose(m.flat_params.cpu().numpy(), p_ref.numpy(), atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize('opt_type', ['Adadelta', 'Adam'])
def test_nan_gradient_skips_step(las, opt_type):
    """solver.py:179-182: `if math.isnan(grad_norm)` -> no optimizer.step(); here the decision is device-side."""
    ops, asr, optim = las
    m, gen = flat_holder(4096, 5)
    opt = optim.FlatOptimizer(m, opt_type, 0.5, eps=1e-8)
    m.flat_grads.copy_(torch.randn(4096, generator=gen).to(DEV))
    opt.step(zero_grad=True)                        # one ordinary step so that the moments are non-trivial
    before = [t.clone() for t in (m.flat_params, opt.s1, opt.s2, opt.step_dev)]
    g = torch.randn(4096, generator=gen)
    g[1234] = float('nan')
    m.flat_grads.copy_(g.to(DEV))
    opt.step(zero_grad=True)
    torch.cuda.synchronize()
    assert float(opt.norm3[2]) == 1.0 and np.isnan(float(opt.norm3[0]))
    for a, b in zip(before, (m.flat_params, opt.s1, opt.s2, opt.step_dev)):
        assert torch.equal(a, b)
    assert float(m.flat_grads.abs().max()) == 0.0   # the gradient buffer is still cleared for the next step


def test_infeasible_ctc_batch_skips_step(las):
    """A label longer than its utterance's T' makes CTCLoss(zero_infinity=False) +inf and its gradient NaN:
    the reference logs 'grad norm is NaN' and skips the update.  Whole step through the HIP path."""
    ops, asr, optim = las
    from gen_golden import TINY
    d = np.load(os.path.join(GOLDEN, 'g3_step_loc_ctc.npz'))
    cfg = TINY['loc_ctc']
    x = torch.tensor(d['x'], device=DEV)
    Tp = int(d['enc_len'].min())
    V = int(d['V'])
    y = torch.zeros(x.shape[0], Tp + 4, dtype=torch.long, device=DEV)
    y[:, 1:Tp + 2] = torch.randint(2, V, (x.shape[0], Tp + 1), device=DEV)      # Tp+1 tokens + <eos> > T'
    y[:, Tp + 2] = 1
    ops.set_precision('f32')
    try:
        model = asr.Seq2Seq(x, V, cfg, device=DEV)
        model.load_reference_state({k[2:]: d[k] for k in d.files if k.startswith('w.')})
        opt = optim.FlatOptimizer(model, 'Adadelta', 1.0, eps=1e-8)
        opt.zero_grad()
        w0 = model.flat_params.clone()
        loss = one_iteration(ops, model, opt, x, y, 0.5)
        torch.cuda.synchronize()
    finally:
        ops.set_precision('bf16')
    assert np.isinf(loss)
    assert float(opt.norm3[2]) == 1.0 and int(opt.step_dev.item()) == 0
    assert torch.equal(w0, model.flat_params)
