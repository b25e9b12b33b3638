"""GPU tests of device-resident evaluation end to end: ``WaveNet.evaluate`` against ``eval_reference`` applied to
``predict`` of the same batches (pred, rank, confusion bit for bit; nll within the 1-ulp bound derived in
tests/test_gpu_eval_entries.py), with eager launches and with graphs, at batch sizes that divide the set, leave a ragged
tail and exceed it; nothing else changes; ``fit(..., validate=...)`` trains the bits of ``fit`` and returns the sweeps
``evaluate`` gives on a model stopped at the same steps; the loss sweeps of the teacher and the auto-encoder against the
host-staged forward-only loss; the example driver.

Shapes: 11 clips of 80 samples, windows of 64, five classes, stacks of three layers [1, 2, 4] at R = 32 and S = 128."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._pkg import ROOT, sub
from tests.eval_reference import eval_reference, ulp_distance

pytestmark = pytest.mark.gpu

N, CLIP, T, C, DIL, R, S = 11, 80, 64, 5, [1, 2, 4], 32, 128
SEED = 3
LABELS = np.arange(N) % C


def _clips(n=N, seed=11):
    rng = np.random.default_rng(seed)
    return (0.9 * np.sin(np.arange(CLIP)[None, :] * rng.uniform(0.05, 0.6, (n, 1))) *
            rng.uniform(0.2, 1.0, (n, 1)) + 0.02 * rng.standard_normal((n, CLIP))).astype(np.float32)


def _classifier(dtype=torch.float32):
    M = sub("model")
    return M.WaveNet(T, C, DIL, dilation_channels=R, skip_channels=S, output_channels=C, learning_rate=1e-3, dtype=dtype,
                     seed=5)


def _held():
    return sub("dataset").DeviceDataset(_clips(), LABELS, C)


def _train_set():
    return sub("dataset").DeviceDataset(_clips(7, seed=12), np.arange(7) % C, C)


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


def _same_result(a, b, nll_bits=True):
    for k in ("pred", "rank", "confusion", "owned", "per_class"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.seen == b.seen and a.accuracy == b.accuracy and a.top_k_accuracy == b.top_k_accuracy
    if nll_bits:
        assert np.array_equal(a.nll.view(np.uint32), b.nll.view(np.uint32))
        assert a.mean_nll == b.mean_nll


def _predict_reference(m, B, crop):
    """``eval_reference`` on ``predict`` of the sweep's own batches (the plan's rows, the wrapped ones of the ragged tail
    included, so the engine sees the batch ``evaluate`` gives it): per-record arrays and the confusion matrix."""
    D = sub("dataset")
    clips = _clips()
    pred, rank = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    nll = np.full(N, np.nan, np.float32)
    conf = np.zeros((C, C), np.int32)
    for s in range(D.sweep_steps(N, B)):
        idx, valid = D.sweep_plan(s, B, N)
        _, off = D.draw_plan(SEED, s, B, N, CLIP, T, False, crop)
        x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        probs = np.ascontiguousarray(m.predict(x)[:, 0, :][valid])
        assert probs.dtype == np.float32
        rec = idx[valid]
        pred[rec], rank[rec], nll[rec], c = eval_reference(probs, LABELS[rec])
        conf += c
    return pred, rank, nll, conf


def _check_against_predict(m, res, B, crop, where):
    pred, rank, nll, conf = _predict_reference(m, B, crop)
    assert res.seen == N and res.owned.all() and res.step is None
    assert np.array_equal(res.pred, pred), where
    assert np.array_equal(res.rank, rank), where
    assert np.array_equal(res.confusion, conf), where
    d = ulp_distance(res.nll, nll)
    print(where, "nll: max ulp distance", int(d.max()), "accuracy", res.accuracy, "mean nll", res.mean_nll)
    assert (d <= 1).all(), where
    assert res.accuracy == float((pred == LABELS).sum()) / N
    assert res.top_k_accuracy == float((rank < res.top_k).sum()) / N
    assert np.array_equal(res.per_class[:, 1], np.bincount(LABELS, minlength=C))
    assert np.array_equal(res.per_class[:, 0], np.bincount(LABELS[pred == LABELS], minlength=C))
    assert res.mean_nll == float(res.nll.astype(np.float64).sum()) / N


# ---- evaluate == predict + the kernel's rules ---------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["0", "1"])
@pytest.mark.parametrize("dtype,crop", [(torch.float32, "head"), (torch.bfloat16, "head"), (torch.float32, "random")])
def test_evaluate_equals_predict(dtype, crop, graphs, monkeypatch):
    """B = 4 on 11 clips: three steps with a ragged tail of three.  The first call runs two eager steps, captures and
    replays once; the second is replays only.  Both return the same bits."""
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", graphs)
    m = _classifier(dtype)
    m.fit(_train_set().sampler(3, T, seed=SEED), 3)          # (a few steps away from the initial posteriors)
    ev = _held().eval_sampler(4, T, crop=crop, seed=SEED, top_k=2)
    assert ev.sweep_steps == 3
    first = m.evaluate(ev)
    st = m._engine(4, T)._eval_state
    assert (st["graph"] is not None) == (graphs == "1") and not st["failed"]
    assert ev.state.cpu().tolist()[1:] == [0, 1] and (ev.step, ev.sweep) == (0, 1)
    _check_against_predict(m, first, 4, crop, "%s %s graphs=%s" % (dtype, crop, graphs))
    second = m.evaluate(ev)
    assert ev.state.cpu().tolist()[1:] == [0, 2]
    _same_result(first, second)


def test_batch_sizes_that_cover_and_exceed_the_set():
    """B = 11 (one full step) and B = 16 (B > N) give the per-record results of B = 4 -- where ``predict`` itself does not
    depend on the batch a clip sits in, which is checked first."""
    D = sub("dataset")
    m = _classifier()
    x = _clips()[:, :T]
    whole = m.predict(x)[:, 0, :]
    plans = [D.sweep_plan(s, 4, N) for s in range(3)]
    parts = np.concatenate([m.predict(x[idx])[:, 0, :][valid] for idx, valid in plans])
    invariant = np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    ds = _held()
    want = m.evaluate(ds.eval_sampler(4, T))
    for B in (11, 16):
        ev = ds.eval_sampler(B, T)
        assert ev.sweep_steps == 1
        got = m.evaluate(ev)
        _check_against_predict(m, got, B, "head", "B=%d" % B)
        if invariant:
            _same_result(got, want)
    if not invariant:
        pytest.skip("predict at B = 4 and B = 11 differ in bits: the comparison across batch sizes was left out")


def test_evaluate_changes_nothing_else():
    m = _classifier()
    s = _train_set().sampler(3, T, seed=SEED)
    m.fit(s, 3)
    before = _snapshot(m, s)
    ev = _held().eval_sampler(4, T)
    m.evaluate(ev)
    m.evaluate(ev)
    m.evaluate(_held().eval_sampler(3, T))                    # the training engine's own batch size
    _same_snapshot(_snapshot(m, s), before)
    assert s.step == 3


# ---- validation inside fit ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stopped():
    """fit(6) without validation, and what evaluate returns on a model stopped after 2, 4 and 6 steps."""
    m = _classifier()
    s = _train_set().sampler(3, T, seed=SEED)
    ev = _held().eval_sampler(4, T)
    losses, results = [], []
    for k in (2, 4, 6):
        losses.append(m.fit(s, 2))
        results.append(m.evaluate(ev, step=k))
    plain = _classifier()
    plain_losses = plain.fit(_train_set().sampler(3, T, seed=SEED), 6)
    assert np.array_equal(np.concatenate(losses).view(np.uint32), plain_losses.view(np.uint32))
    return dict(losses=plain_losses, params=_snapshot(plain), results=results)


@pytest.mark.parametrize("capacity", [16, 2])
def test_fit_with_validation(stopped, capacity):
    """The training run keeps its bits; three sweeps come back with steps 2, 4 and 6, each what ``evaluate`` returns on a
    model stopped there.  With two slots the run drains in between and still returns all three."""
    m = _classifier()
    s = _train_set().sampler(3, T, seed=SEED)
    ev = _held().eval_sampler(4, T, sweep_capacity=capacity)
    losses, results = m.fit(s, 6, validate=(ev, 2))
    assert losses.dtype == np.float32 and np.array_equal(losses.view(np.uint32), stopped["losses"].view(np.uint32))
    _same_snapshot(_snapshot(m), stopped["params"])
    assert [r.step for r in results] == [2, 4, 6] and ev.sweep == 3
    for got, want in zip(results, stopped["results"]):
        _same_result(got, want)
    assert isinstance(m.fit(s, 1), np.ndarray)                 # without validate: the losses alone, as before
    more, after = m.fit(s, 1, validate=(ev, 2))                # step 8: the count is the sampler's, not the call's
    assert [r.step for r in after] == [8] and more.shape == (1,)


def test_validation_on_the_training_engine(stopped):
    """Sweeps at the training batch size run on the training step's own engine, between its graph's replays: the run
    still keeps its bits, and the sweeps are the ones ``evaluate`` gives there."""
    m = _classifier()
    s = _train_set().sampler(3, T, seed=SEED)
    ev = _held().eval_sampler(3, T)
    assert m._engine(3, T) is m._engine(ev.batch_size, ev.num_samples)
    losses, results = m.fit(s, 6, validate=(ev, 2))
    assert np.array_equal(losses.view(np.uint32), stopped["losses"].view(np.uint32))
    _same_snapshot(_snapshot(m), stopped["params"])
    assert [r.step for r in results] == [2, 4, 6] and all(r.seen == N for r in results)
    final = m.evaluate(ev)
    _same_result(results[-1], final)
    _check_against_predict(m, final, 3, "head", "validation at the training batch size")


# ---- the loss sweeps ----------------------------------------------------------------------------------------------------
def test_teacher_evaluate_equals_loss():
    M, D = sub("model"), sub("dataset")
    clips = _clips(8)[:, :T]
    m = M.WaveNetTeacher(T, 0, DIL, dilation_channels=R, skip_channels=S, quantization_channels=256, dtype=torch.float32,
                         learning_rate=1e-3, seed=5)
    want = np.array([m.loss(clips[i:i + 4]) for i in (0, 4)], np.float32)
    before = _snapshot(m)
    s = D.DeviceDataset(clips).sampler(4, T, shuffle=False)
    for _ in range(2):                                         # eager steps and the capture, then replays
        got = m.evaluate(s)
        assert got.dtype == np.float32 and got.shape == (2,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    _same_snapshot(_snapshot(m), before)


def test_autoencoder_evaluate_equals_the_staged_loss():
    """The auto-encoder case of tests/test_gpu_dataset.py: 64 samples, four condition classes, five mixtures, bf16,
    batches of 2."""
    M, D = sub("model"), sub("dataset")
    clips = _clips(8)[:, :T]
    labels = np.arange(8) % 4
    m = M.WaveNetAutoEncoder(T, 4, 5, DIL, dilation_channels=R, skip_channels=S, latent_channels=8, pool_stride=16,
                             learning_rate=1e-3, dtype=torch.bfloat16, seed=5)
    want = []
    for i in range(0, 8, 2):
        eng = m._stage(clips[i:i + 2], np.eye(4, dtype=np.float32)[labels[i:i + 2]])
        eng.forward()
        want.append(eng.loss.item())
    want = np.array(want, np.float32)
    params = {k: v.detach().clone() for k, v in m.network_params.items()}
    s = D.DeviceDataset(clips, labels, 4).sampler(2, T, shuffle=False)
    for _ in range(2):
        got = m.evaluate(s)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    for k, v in m.network_params.items():
        assert torch.equal(v, params[k]), k


# ---- the example driver -------------------------------------------------------------------------------------------------
def test_classifier_driver_runs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "classifier.py"), "--train", "--device-data", "--test",
                        "--steps", "4", "--num-samples", "256", "--layers", "3", "--batch-size", "2", "--print-steps", "2",
                        "--device-clips", "6", "--validation-clips", "5", "--validate-every", "2", "--eval-batch-size", "4",
                        "--test-clips", "9", "--seed", "0", "--logdir", str(tmp_path / "run")],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ), cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(re.findall(r"Validation: \d+ of 5 ", r.stdout)) == 2, r.stdout[-2000:]
    tot = re.search(r"Correct: (\d+) \| Wrong: (\d+) \| Total: (\d+) \| % Correct: ([0-9.]+)", r.stdout)
    assert tot, r.stdout[-2000:]
    correct, wrong, total = (int(tot.group(i)) for i in (1, 2, 3))
    assert total == 9 and correct + wrong == 9
    per = {k: eval(v) for k, v in re.findall(r"^(Correct|Wrongs) (\{.*\})$", r.stdout, flags=re.M)}
    assert sum(per["Correct"].values()) == correct and sum(per["Wrongs"].values()) == wrong
    assert os.path.exists(tmp_path / "run" / "checkpoint")
