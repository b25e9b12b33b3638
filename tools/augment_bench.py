#!/usr/bin/env python3
"""What augmenting the drawn batch costs on one MI355X: the draw launch alone, and a whole ``fit`` step.

Launches, at 8 x 16000 out of 64 clips of 16000 (crop "head") into one audio buffer and the codes -- microseconds per launch
of ``srwn_batch_draw`` against ``srwn_batch_draw_aug`` with a shift only (+-1600), a gain only (0.7 .. 1.3) and all three
(the shift, the gain, 8 noise clips of 16000 + 4000 samples mixed into every row at 0.1 .. 0.5), and against
``srwn_batch_draw_warp`` with a speed only (0.9 .. 1.1, 16 taps) and with all three behind it, and against
``srwn_batch_draw_room`` with every row convolved with one of 8 synthetic room responses of 512, 2048 and 8192 taps, all
three behind it, without and with the speed -- each beside the floor of the vector units for its 2 B T K operations,
``2 B T K / (16 384 lanes x clock)`` at --clock-ghz, and half that where multiply and add are issued packed:

  warm   a hipGraph of --launches launches of one draw replayed: best of --reps replays, per launch
  cold   the same replay right after a 512 MiB buffer has been rewritten, so that clips and noise come from HBM again

Steps, for the config-2 teacher (30 layers, R = 64, S = 256, softmax, bf16, batch 8 x 16000) and examples/classifier.py's
network (20 layers, 32 / 128 channels, 4 classes, batch --classifier-batch x 16384) -- milliseconds per step, best of
--reps regions of --steps steps with the spread (tools/fit_bench.py's regions), after a warm-up that includes the capture:

  (a) fit            model.fit(sampler, steps), no augmentation
  (b) fit, augmented the same with augment=Augment(all three)
  (c) host loop      dataset.augment_rows in NumPy over the plans' rows, then model.train(x)
  (d) fit, resampled (b) with speed=(0.9, 1.1): the draw is srwn_batch_draw_warp
  (e) host loop      dataset.resample_rows, then dataset.augment_rows, then model.train(x)
  (f) fit, reverberated (d) with every row convolved with one of 8 responses of --room-taps taps: srwn_batch_draw_room
  (g) host loop      dataset.resample_rows, dataset.reverb_rows, dataset.augment_rows, then model.train(x); regions of
                     --host-room-steps steps (a row of 16000 samples under 4096 taps is tens of milliseconds in NumPy)

usage: python tools/augment_bench.py [--steps 100] [--reps 3] [--only launches|teacher|classifier]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
RECORDS, NOISE_CLIPS, NOISE_EXTRA = 64, 8, 4000
SPEED = (0.9, 1.1)
RIRS, ROOM_TAPS = 8, (512, 2048, 8192)
LANES = 16384                    # 256 compute units x 64 fp32 lanes


def make_clips(n, length, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float32)[None, :]
    return (0.5 * np.sin(t * rng.uniform(0.01, 0.3, (n, 1))) + 0.05 * rng.standard_normal((n, length))).astype(np.float32)


def settings(D, T, noise):
    return {"shift only": D.Augment(shift=T // 10), "gain only": D.Augment(gain=(0.7, 1.3)),
            "all three": D.Augment(shift=T // 10, gain=(0.7, 1.3), noise=noise, noise_prob=1.0, noise_volume=(0.1, 0.5)),
            "speed only": D.Augment(speed=SPEED),
            "speed, all three": D.Augment(shift=T // 10, gain=(0.7, 1.3), noise=noise, noise_prob=1.0, noise_volume=(0.1, 0.5),
                                          speed=SPEED)}


def room_settings(D, T, noise, taps, speed, prob=1.0):
    rirs = D.DeviceDataset(D.synthetic_rirs(RIRS, taps, rt60=(0.2, 0.6), seed=3))
    return D.Augment(shift=T // 10, gain=(0.7, 1.3), noise=noise, noise_prob=1.0, noise_volume=(0.1, 0.5),
                     speed=SPEED if speed else (1.0, 1.0), reverb=rirs, reverb_prob=prob)


def regions(run, steps, reps):
    """ms per step of `reps` regions of `steps` steps: (best, spread)."""
    import torch
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) / steps * 1e3)
    return min(v), max(v) - min(v)


def launches(a):
    import torch
    D = importlib.import_module("sr-wavenet_amd.dataset")
    B, T = 8, 16000
    data = D.DeviceDataset(make_clips(RECORDS, T))
    noise = D.DeviceDataset(make_clips(NOISE_CLIPS, T + NOISE_EXTRA, seed=1))
    audio = torch.zeros((B, T), device="cuda")
    codes = torch.zeros(B * T, dtype=torch.int32, device="cuda")
    flush = torch.zeros(512 << 18, device="cuda")                   # 512 MiB: more than the caches hold
    print("== draw launches, %d x %d: us per launch, best of %d (spread); warm = %d launches per replay" % (B, T, a.reps, a.launches))
    cases = [("srwn_batch_draw", None)] + [("srwn_batch_draw_%s, %s" % ("warp" if v.resamples else "aug", k), v)
                                           for k, v in settings(D, T, noise).items()]
    cases += [("srwn_batch_draw_room, K = %d%s" % (k, ", speed" if sp else ""), room_settings(D, T, noise, k, sp))
              for k in ROOM_TAPS for sp in (False, True)]
    for name, aug in cases:
        s = data.sampler(B, T, seed=0, augment=aug)
        s.draw(audio, codes=codes, quantization_channels=256)
        torch.cuda.synchronize()
        many, one = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(many):
            for _ in range(a.launches):
                s.draw(audio, codes=codes, quantization_channels=256)
        with torch.cuda.graph(one):
            s.draw(audio, codes=codes, quantization_channels=256)
        many.replay()
        warm = regions(lambda n: many.replay(), 1, a.reps)
        cold = []
        for _ in range(a.reps):
            flush.add_(1.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one.replay()
            torch.cuda.synchronize()
            cold.append((time.perf_counter() - t0) * 1e6)
        floor = ""
        if aug is not None and aug.reverberates:
            us = 2.0 * B * T * aug.reverb.clip_len / (LANES * a.clock_ghz * 1e3)
            floor = "   VALU floor %.2f, packed %.2f" % (us, us / 2)
        print("   %-36s warm %8.2f (%.2f)   cold, with the replay's own launch cost %8.2f (%.2f)%s"
              % (name, warm[0] * 1e3 / a.launches, warm[1] * 1e3 / a.launches, min(cold), max(cold) - min(cold), floor),
              flush=True)


def steps(a, kind):
    import gc
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    D = importlib.import_module("sr-wavenet_amd.dataset")
    if kind == "teacher":
        B, T, classes = 8, 16000, 0
        make = lambda: M.WaveNetTeacher(T, 0, DIL, dilation_channels=64, skip_channels=256, quantization_channels=256)
    else:
        B, T, classes = a.classifier_batch, 16384, 4
        make = lambda: M.WaveNet(T, classes, DIL[:20], dilation_channels=32, skip_channels=128, output_channels=classes,
                                 learning_rate=0.001)                                        # examples/classifier.py
    clips = make_clips(RECORDS, T)
    nz = make_clips(NOISE_CLIPS, T + NOISE_EXTRA, seed=1)
    labels = (np.arange(RECORDS) % classes) if classes else None
    data = D.DeviceDataset(clips, labels, classes)
    aug = settings(D, T, D.DeviceDataset(nz))["all three"]
    warp = settings(D, T, aug.noise)["speed, all three"]
    print("== %s, batch %d x %d: ms per step, best of %d regions of %d steps (spread)" % (kind, B, T, a.reps, a.steps), flush=True)
    out = {}
    room = room_settings(D, T, aug.noise, a.room_taps, True)
    rirs = room.reverb.audio.cpu().numpy()
    for key, augment in (("a", None), ("b", aug), ("d", warp), ("f", room)):
        m = make()
        s = data.sampler(B, T, seed=0, augment=augment)
        m.fit(s, a.warmup)
        out[key] = regions(lambda n: m.fit(s, n), a.steps, a.reps)
        del m, s
        gc.collect()
        torch.cuda.empty_cache()
    m = make()
    eye = np.eye(max(classes, 1), dtype=np.float32)
    st = [0]

    def host(n, resample=False, reverb=False):
        for _ in range(n):
            idx, off = D.draw_plan(0, st[0], B, RECORDS, T, T)
            plan = D.augment_plan(0, st[0], B, T, aug, NOISE_CLIPS, T + NOISE_EXTRA)
            x = clips[idx]
            if resample:
                x = D.resample_rows(x, D.speed_plan(0, st[0], B, warp), warp.table())
            if reverb:
                x = D.reverb_rows(x, D.reverb_plan(0, st[0], B, room, RIRS), rirs)
            x = D.augment_rows(x, plan, nz)
            m.train(x, eye[labels[idx]]) if classes else m.train(x)
            st[0] += 1
    host(a.warmup)
    out["c"] = regions(host, a.steps, a.reps)
    out["e"] = regions(lambda n: host(n, True), a.steps, a.reps)
    out["g"] = regions(lambda n: host(n, True, True), a.host_room_steps, a.reps)
    for key, name in (("a", "(a) fit"), ("b", "(b) fit, augmented"), ("c", "(c) host loop: augment_rows, train(x)"),
                      ("d", "(d) fit, resampled and augmented"), ("e", "(e) host loop: resample_rows, augment_rows, train(x)"),
                      ("f", "(f) fit, resampled, reverberated (K = %d), augmented" % a.room_taps),
                      ("g", "(g) host loop: resample_rows, reverb_rows, augment_rows, train(x)")):
        print("   %-68s %.4f (%.4f)" % (name, *out[key]), flush=True)
    print("   (b) - (a) = %+.4f ms   (c) - (b) = %+.4f ms   (d) - (a) = %+.4f ms   (e) - (d) = %+.4f ms   (f) - (a) = %+.4f ms"
          "   (g) - (f) = %+.4f ms"
          % (out["b"][0] - out["a"][0], out["c"][0] - out["b"][0], out["d"][0] - out["a"][0], out["e"][0] - out["d"][0],
             out["f"][0] - out["a"][0], out["g"][0] - out["f"][0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--classifier-batch", type=int, default=1, help="examples/classifier.py's default")
    ap.add_argument("--room-taps", type=int, default=4096, help="taps of the room responses of the fit steps")
    ap.add_argument("--host-room-steps", type=int, default=2, help="steps per region of the reverberating host loop")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock of the VALU floor")
    ap.add_argument("--only", default=None, choices=["launches", "teacher", "classifier"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    for what in ([a.only] if a.only else ["launches", "teacher", "classifier"]):
        launches(a) if what == "launches" else steps(a, what)


if __name__ == "__main__":
    main()
