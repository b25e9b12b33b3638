"""GPU tests of device-resident evaluation of the twin towers and the student end to end.

``SiameseWaveNet.evaluate``: the embeddings it returns equal ``get_embedding`` of the sweep's own batches bit for bit (fp32
and bf16, eager launches and graphs, batch sizes that leave a ragged tail, cover the set and exceed it); the result equals
``pair_reference`` applied to the stored matrix, which is ``srwn_gallery_match`` of those embeddings; nothing else changes.
``fit(..., validate=...)`` trains the bits of ``fit`` and returns the sweeps ``evaluate`` gives on a model stopped at the
same steps, also with more sweeps than result slots.  ``ParallelWaveNet.evaluate`` equals the host loop (``encode``,
``noise_plan``, the staged forward pass, ``losses()``) bit for bit and changes nothing else.  The example driver.

Twins: the shapes of tests/test_gpu_evaluate.py -- 11 clips of 80 samples, windows of 64, three layers [1, 2, 4] at R = 32
and S = 128 --, D in {2, 5}, four classes of which the last has a single member.  Student: those of
tests/test_gpu_fit_pairs.py on 6 clips."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._pkg import ROOT, sub
from tests.pair_eval_reference import distance_matrix_fp64, pair_reference

pytestmark = pytest.mark.gpu

N, CLIP, T, C, DIL, R, S = 11, 80, 64, 4, [1, 2, 4], 32, 128
SEED, BINS, P = 3, 16, 3
LABELS = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 3])                # class 3: one member
COUNTED = ("nearest", "nearest_dist", "same_nearest", "same_dist", "rank_same", "hist_same", "hist_diff")


def _clips(n=N, seed=11, length=CLIP):
    rng = np.random.default_rng(seed)
    return (0.9 * np.sin(np.arange(length)[None, :] * rng.uniform(0.05, 0.6, (n, 1))) *
            rng.uniform(0.2, 1.0, (n, 1)) + 0.02 * rng.standard_normal((n, length))).astype(np.float32)


def _twins(dim=2, dtype=torch.float32):
    return sub("model").SiameseWaveNet(T, dim, DIL, margin=0.5, dilation_channels=R, skip_channels=S, learning_rate=1e-3,
                                       dtype=dtype, seed=5)


def _held():
    return sub("dataset").DeviceDataset(_clips(), LABELS, C)


def _train_set():
    return sub("dataset").DeviceDataset(_clips(9, seed=12), np.array([0, 1, 0, 2, 1, 0, 3, 1, 0]), C)


def _snapshot(m, sampler=None):
    e = m._primary
    out = dict(params=e.params.clone(), adam_m=e.adam_m.clone(), adam_v=e.adam_v.clone(), adam_step=e.adam_step.clone(),
               packed=e.packed.clone())
    if sampler is not None:
        out["sampler"] = sampler.state.clone()
    return out


def _same_snapshot(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_result(a, b):
    for k in COUNTED + ("emb", "labels"):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    assert a.seen == b.seen and a.bins == b.bins and a.d_max == b.d_max
    for k in ("nn_accuracy", "eer", "eer_threshold", "auc"):
        assert getattr(a, k) == getattr(b, k) or (np.isnan(getattr(a, k)) and np.isnan(getattr(b, k))), k


def _gallery(emb):
    K = sub("kernels")
    n, dim = emb.shape
    e = torch.as_tensor(emb, device="cuda")
    ng = torch.tensor([n], dtype=torch.int32, device="cuda")
    dist = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    near = torch.zeros(n, dtype=torch.int32, device="cuda")
    dmin = torch.zeros(n, dtype=torch.float32, device="cuda")
    K.call("srwn_gallery_match", e.data_ptr(), n, dim, e.data_ptr(), ng.data_ptr(), n, dist.data_ptr(), near.data_ptr(),
           dmin.data_ptr(), K._stream())
    return dist.cpu().numpy()


def _embedding_reference(m, B, crop):
    """``get_embedding`` of the sweep's own batches (the plan's rows, the wrapped ones of the ragged tail included, so the
    engine sees the batch ``evaluate`` gives it), each valid row at its record."""
    D = sub("dataset")
    clips = _clips()
    emb = np.full((N, m.output_dimensions), np.nan, np.float32)
    for s in range(D.sweep_steps(N, B)):
        idx, valid = D.sweep_plan(s, B, N)
        _, off = D.draw_plan(SEED, s, B, N, CLIP, T, False, crop)
        x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        e = m.get_embedding(None, x)[:, 0, :]
        assert e.dtype == np.float32
        emb[idx[valid]] = e[valid]
    assert np.isfinite(emb).all()
    return emb


def _check_result(m, res, B, crop, where):
    emb = _embedding_reference(m, B, crop)
    assert res.seen == N and res.step is None and np.array_equal(res.labels, LABELS)
    assert np.array_equal(_bits(res.emb), _bits(emb)), where
    # the matrix rule of tests/test_gpu_pair_eval_entries.py: the gallery's bits, symmetric, within the bound of float64
    dist = res.distances
    assert dist is not None and dist.shape == (N, N) and dist.dtype == np.float32
    assert np.array_equal(_bits(dist), _bits(_gallery(emb))), where
    assert np.array_equal(_bits(dist), _bits(dist.T.copy()))
    d64, bound = distance_matrix_fp64(emb)
    assert (np.abs(dist.astype(np.float64) - d64) <= bound).all()
    assert res.d_max == 2.0 * m.margin and res.bins == BINS
    want = pair_reference(dist, LABELS, BINS, np.float32(BINS / res.d_max))
    for k, w in zip(COUNTED, want):
        assert np.array_equal(_bits(getattr(res, k)), _bits(w)), "%s: %s" % (where, k)
    assert res.same_nearest[10] == -1 and res.rank_same[10] == -1 and res.same_dist[10] == np.inf
    assert int(res.hist_same.sum()) == 6 + 3 + 3 and int(res.hist_same.sum() + res.hist_diff.sum()) == N * (N - 1) // 2
    assert res.nn_accuracy == float((res.rank_same == 0).sum()) / N == res.recall_at(1)
    assert res.recall_at(3) == float(((res.rank_same >= 0) & (res.rank_same < 3)).sum()) / N
    far, frr = res.rates()
    assert far[0] == 0 and frr[0] == 1 and far[-1] == 1 and frr[-1] == 0 and 0.0 <= res.eer <= 1.0 and 0.0 <= res.auc <= 1.0
    print(where, res)


# ---- evaluate == get_embedding + the kernel's rules ---------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["0", "1"])
@pytest.mark.parametrize("dtype,dim,B,crop", [(torch.float32, 2, 4, "head"), (torch.bfloat16, 2, 4, "head"),
                                              (torch.float32, 5, 4, "random"), (torch.float32, 5, 11, "head"),
                                              (torch.bfloat16, 5, 16, "head"), (torch.float32, 2, 16, "head"),
                                              (torch.bfloat16, 2, 11, "random")])
def test_evaluate_equals_get_embedding(dtype, dim, B, crop, graphs, monkeypatch):
    """B = 4 on 11 clips: three steps with a ragged tail of three (two eager steps, the capture, one replay; a second call
    is replays only); B = 11: one full step; B = 16: B > N.  Both calls return the same bits."""
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", graphs)
    m = _twins(dim, dtype)
    m.fit(_train_set().pair_sampler(P, T, seed=SEED), 3)         # (a few steps away from the initial embedding)
    es = _held().embed_sampler(B, T, crop=crop, seed=SEED, bins=BINS)
    assert es.sweep_steps == -(-N // B) and es.d_max is None
    first = m.evaluate(es, distances=True)
    assert es.state.cpu().tolist()[1:] == [0, 1] and (es.step, es.sweep) == (0, 1)
    _check_result(m, first, B, crop, "%s D=%d B=%d %s graphs=%s" % (dtype, dim, B, crop, graphs))
    second = m.evaluate(es)
    assert second.distances is None and es.state.cpu().tolist()[1:] == [0, 2]
    _same_result(first, second)
    third = m.evaluate(es, step=7)
    st = m._engine(B, T)._eval_state
    assert (st["graph"] is not None) == (graphs == "1") and not st["failed"] and third.step == 7
    _same_result(first, third)


def test_evaluate_changes_nothing_else():
    m = _twins()
    s = _train_set().pair_sampler(P, T, seed=SEED)
    m.fit(s, 3)
    before = _snapshot(m, s)
    es = _held().embed_sampler(4, T, bins=BINS)
    m.evaluate(es)
    m.evaluate(es, distances=True)
    m.evaluate(_held().embed_sampler(2 * P, T, bins=BINS))      # the training engine's own batch size
    _same_snapshot(_snapshot(m, s), before)
    assert s.step == 3
    loss, dist = m.fit(s, 1)                                     # ... and training goes on from there
    assert np.isfinite(loss).all() and s.step == 4


def test_a_d_max_of_the_samplers_own_stays():
    m = _twins()
    es = _held().embed_sampler(4, T, bins=BINS, d_max=0.25)
    res = m.evaluate(es, distances=True)
    assert res.d_max == 0.25 and es.d_max == 0.25
    want = pair_reference(res.distances, LABELS, BINS, np.float32(BINS / 0.25))
    for k, w in zip(COUNTED, want):
        assert np.array_equal(_bits(getattr(res, k)), _bits(w)), k
    with pytest.raises(ValueError, match="bound to 2 embedding dimensions, the model has 5"):
        _twins(5).evaluate(es)


# ---- validation inside fit ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stopped():
    """fit(6) without validation, and what evaluate returns on a model stopped after 2, 4 and 6 steps."""
    m = _twins()
    s = _train_set().pair_sampler(P, T, seed=SEED)
    es = _held().embed_sampler(4, T, bins=BINS)
    loss, dist, results = [], [], []
    for k in (2, 4, 6):
        l, d = m.fit(s, 2)
        loss.append(l); dist.append(d)
        results.append(m.evaluate(es, step=k))
    plain = _twins()
    plain_loss, plain_dist = plain.fit(_train_set().pair_sampler(P, T, seed=SEED), 6)
    assert np.array_equal(_bits(np.concatenate(loss)), _bits(plain_loss))
    assert np.array_equal(_bits(np.concatenate(dist)), _bits(plain_dist))
    return dict(loss=plain_loss, dist=plain_dist, params=_snapshot(plain), results=results)


@pytest.mark.parametrize("capacity", [4, 2])
def test_fit_with_validation(stopped, capacity):
    """The training run keeps its bits; three sweeps come back with steps 2, 4 and 6, each what ``evaluate`` returns on a
    model stopped there.  With two slots the run holds more sweeps than slots: it drains in between and returns all three."""
    m = _twins()
    s = _train_set().pair_sampler(P, T, seed=SEED)
    es = _held().embed_sampler(4, T, bins=BINS, sweep_capacity=capacity)
    loss, dist, results = m.fit(s, 6, validate=(es, 2))
    assert loss.dtype == np.float32 and np.array_equal(_bits(loss), _bits(stopped["loss"]))
    assert np.array_equal(_bits(dist), _bits(stopped["dist"]))
    _same_snapshot(_snapshot(m), stopped["params"])
    assert [r.step for r in results] == [2, 4, 6] and es.sweep == 3
    for got, want in zip(results, stopped["results"]):
        _same_result(got, want)
    assert len(m.fit(s, 1)) == 2                                 # without validate: (loss, distance), as before
    more, _, after = m.fit(s, 1, validate=(es, 2))               # step 8: the count is the sampler's, not the call's
    assert [r.step for r in after] == [8] and more.shape == (1,)


def test_validation_on_the_training_engine(stopped):
    """Sweeps at the training batch size (2P rows) run on the training step's own engine, between its graph's replays."""
    m = _twins()
    s = _train_set().pair_sampler(P, T, seed=SEED)
    es = _held().embed_sampler(2 * P, T, bins=BINS)
    assert m._engine(2 * P, T) is m._engine(es.batch_size, es.num_samples)
    loss, dist, results = m.fit(s, 6, validate=(es, 2))
    assert np.array_equal(_bits(loss), _bits(stopped["loss"])) and np.array_equal(_bits(dist), _bits(stopped["dist"]))
    _same_snapshot(_snapshot(m), stopped["params"])
    assert [r.step for r in results] == [2, 4, 6] and all(r.seen == N for r in results)
    _same_result(results[-1], m.evaluate(es, step=6))


# ---- the student --------------------------------------------------------------------------------------------------------
SN, SCLIP, SB, ST, LAT, POOL, NC = 6, 800, 2, 768, 8, 64, 4
SLABELS = np.array([0, 3, -1, 1, 2, NC], np.int64)               # labels 2 and 5 lie outside the classes: zero conditions


def _onehot(labels, width):
    out = np.zeros((len(labels), width), np.float32)
    ok = (labels >= 0) & (labels < width)
    out[np.nonzero(ok)[0], labels[ok]] = 1.0
    return out


def _student(tmp, dtype, cs):
    M = sub("model")
    t = M.WaveNetAutoEncoder(ST, cs, 5, DIL, dilation_channels=R, skip_channels=S, latent_channels=LAT, pool_stride=POOL,
                             learning_rate=1e-3, dtype=dtype, seed=5)
    t._engine(SB, ST)
    t.save(str(tmp), 0, force=True)
    return M.ParallelWaveNet(ST, cs, DIL, str(tmp), num_flows=2, dilation_channels=R, skip_channels=S, latent_channels=LAT,
                             pool_stride=POOL, learning_rate=1e-3, dtype=dtype, seed=7)


def _noise(step):
    D, K = sub("dataset"), sub("kernels")
    k = D.noise_plan(SEED, step, SB, ST)
    bits = torch.as_tensor(k.astype(np.int64), device="cuda").to(torch.int32).contiguous()
    out = torch.empty((SB, ST), device="cuda")
    K.call("srwn_logistic_from_bits", bits.data_ptr(), out.data_ptr(), bits.numel(), K._stream())
    return out.cpu().numpy()


def _student_state(m):
    e = m._primary
    out = {"flows/" + k: v.detach().clone() for k, v in m.network_params.items()}
    out.update({"teacher/" + k: v.detach().clone() for k, v in m._teacher.network_params.items()})
    out.update(adam_m=e.storage.adam_m.clone(), adam_v=e.storage.adam_v.clone(), adam_step=e.storage.adam_step.clone())
    return out


@pytest.mark.parametrize("dtype,cs", [(torch.float32, 0), (torch.bfloat16, NC)], ids=["fp32-plain", "bf16-conditioned"])
def test_student_evaluate_equals_the_host_loop(tmp_path, dtype, cs):
    D = sub("dataset")
    clips = _clips(SN, length=SCLIP)
    m = _student(tmp_path, dtype, cs)
    ds = D.DeviceDataset(clips, SLABELS if cs else None, NC if cs else 0)
    train = ds.distill_sampler(SB, ST, seed=SEED, crop="random")
    m.fit(train, 3)                                              # (a few steps away from the initial flows)
    want = []
    for s in range(SN // SB):
        idx, off = D.draw_plan(SEED, s, SB, SN, SCLIP, ST, False, "random")
        assert idx.tolist() == [s * SB, s * SB + 1]
        x = np.stack([clips[i, o:o + ST] for i, o in zip(idx, off)])
        c = _onehot(SLABELS[idx], NC) if cs else None
        eng = m._stage(_noise(s), x, m.encode(None, x, c), c)
        eng.forward()
        l = eng.losses()
        want.append([np.float32(l["loss"]), np.float32(l["power_loss"]), np.float32(l["entropy"])])
    want = np.array(want, np.float32).T
    before = _student_state(m)
    tstate = train.state.clone()
    held = ds.distill_sampler(SB, ST, seed=SEED, shuffle=False, crop="random")
    for call in range(2):                                        # eager steps and the capture, then replays
        got = m.evaluate(held)
        assert len(got) == 3 and all(g.dtype == np.float32 and g.shape == (SN // SB,) for g in got)
        print("evaluate", [g.tolist() for g in got], "host loop", want.tolist())
        for g, w, name in zip(got, want, ("loss", "power_loss", "entropy")):
            assert np.array_equal(_bits(g), _bits(w)), "call %d: %s" % (call, name)
    assert m._engine(SB, ST)._eval_state["graph"] is not None
    after = _student_state(m)
    assert set(after) == set(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    assert torch.equal(train.state, tstate) and train.step == 3
    short = m.evaluate(ds.distill_sampler(SB, ST, seed=SEED, shuffle=False, crop="random", log_capacity=2))
    for g, w in zip(short, want):                                # a ring shorter than the sweep drains in between
        assert np.array_equal(_bits(g), _bits(w))
    loss, _ = m.fit(train, 1)                                    # ... and training goes on from there
    assert np.isfinite(loss).all() and train.step == 4


# ---- the example driver -------------------------------------------------------------------------------------------------
def test_siamese_driver_sweeps_a_held_out_set(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "siamese.py"), "--train", "--device-data", "--test",
                        "--steps", "4", "--num-samples", "256", "--layers", "3", "--batch-size", "2", "--print-steps", "2",
                        "--device-clips", "8", "--test-clips", "13", "--eval-batch-size", "4", "--bins", "32", "--seed", "0",
                        "--logdir", str(tmp_path / "run")],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ), cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    held = re.search(r"Held-out: (\d+) clips \| pairs: (\d+) same, (\d+) different", r.stdout)
    assert held, r.stdout[-2000:]
    assert int(held.group(1)) == 13 and int(held.group(2)) + int(held.group(3)) == 13 * 12 // 2
    nn = re.search(r"1-NN accuracy: ([0-9.]+) \| recall@5: ([0-9.]+) \| recall@10: ([0-9.]+)", r.stdout)
    assert nn and 0.0 <= float(nn.group(1)) <= float(nn.group(2)) <= float(nn.group(3)) <= 1.0, r.stdout[-2000:]
    assert re.search(r"EER: ([0-9.]+|nan) at distance ([0-9.]+|nan) .* AUC: ([0-9.]+|nan)", r.stdout), r.stdout[-2000:]
    assert os.path.exists(tmp_path / "run" / "checkpoint")
