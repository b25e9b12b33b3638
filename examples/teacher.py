#!/usr/bin/env python3
"""Parallel driver to the reference's teacher.py (train / reconstruct / checkpoint loop, teacher.py:27-112) on the
MI355X implementation: same model calls, no TensorFlow session, no plotting.

  python examples/teacher.py --teacher runs/teacher --steps 200                    # synthetic waves (simple_audio)
  python examples/teacher.py --teacher runs/teacher --tfrecord nsynth.tfrecord     # NSynth clips (nsynth.py)
  python examples/teacher.py --teacher runs/teacher --tfrecord nsynth.tfrecord --device-data
                                            # the clips loaded onto the device once, every batch drawn there (dataset.py)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-wavenet_amd", "dropin"))
import numpy as np                                   # noqa: E402
from model import WaveNetAutoEncoder                 # noqa: E402  (the dropin shim -> sr-wavenet_amd.model)
from nsynth import NsynthDataReader                  # noqa: E402
from simple_audio import generate_wave_batch         # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--teacher", type=str, default="teachers/%d" % int(time.time() * 1000))
    p.add_argument("--tfrecord", type=str, default=None, help="NSynth TFRecord file; default: synthetic waves")
    p.add_argument("--audio-max-length", type=int, default=16000)
    p.add_argument("--latent-channels", type=int, default=16)
    p.add_argument("--pool-stride", type=int, default=512)
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--num-samples", type=int, default=4096)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--print-steps", type=int, default=50)
    p.add_argument("--layers", type=int, default=30)
    p.add_argument("--device-data", action="store_true",
                   help="keep the clips on the device and draw every batch inside the training step (model.fit)")
    p.add_argument("--device-clips", type=int, default=256, help="--device-data without --tfrecord: synthetic waves to hold")
    import importlib
    O = importlib.import_module("sr-wavenet_amd.optim")
    O.add_control_flags(p)
    a = p.parse_args(argv)
    dilations = ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3)[:a.layers]
    data = NsynthDataReader(a.tfrecord, a.batch_size, a.num_samples, audio_max_length=a.audio_max_length) if a.tfrecord else None
    teacher = WaveNetAutoEncoder(input_size=a.num_samples, condition_size=0, num_mixtures=5, dilations=dilations,
                                 latent_channels=a.latent_channels, skip_channels=128, pool_stride=a.pool_stride,
                                 learning_rate=1e-4)                                     # teacher.py:61
    O.apply_control_flags(teacher, a, 1e-4, a.steps)
    teacher.load(a.teacher)
    if a.device_data:
        return fit_loop(a, teacher)
    loss = None
    first = teacher.training_step() if a.resume and teacher.load_training_state(a.teacher) else 0
    for step in range(first, a.steps):
        x = data.next()[0] if data else generate_wave_batch(a.batch_size, a.num_samples)[0].astype(np.float32)
        loss = teacher.train(x, None)                                                     # teacher.py:78
        if step % a.print_steps == 0:
            regen = teacher.reconstruct(x, None); enc = teacher.encode(x, None)           # teacher.py:83-84
            print(step, float(loss), "reconstruction rms %.3f" % float(np.sqrt(np.mean(regen ** 2))), "encoding", enc.shape, flush=True)
        if teacher.save(a.teacher, step, force=False) and a.resume:                       # once per minute, teacher.py:110
            teacher.save_training_state(a.teacher, step)
    teacher.save(a.teacher, a.steps - 1, force=True)
    if a.resume:
        teacher.save_training_state(a.teacher, a.steps - 1)
    return None if loss is None else float(loss)


def fit_loop(a, teacher):
    """--device-data: the TFRecord file (or a block of synthetic waves) is loaded onto the device once; the steps between
    two prints are one ``fit`` call -- graph replays with no upload, one host wait for the losses."""
    import importlib
    D = importlib.import_module("sr-wavenet_amd.dataset")
    if a.tfrecord:
        data = D.DeviceDataset.from_tfrecord(a.tfrecord, a.audio_max_length, label_key=None)
    else:
        data = D.DeviceDataset(generate_wave_batch(a.device_clips, a.num_samples)[0].astype(np.float32))
    sampler = data.sampler(a.batch_size, a.num_samples, seed=0)
    print("%d clips of %d samples on the device (%.1f MB)" % (len(data), data.clip_len, data.nbytes / 1e6), flush=True)
    loss, step = None, 0
    if a.resume and teacher.load_training_state(a.teacher, sampler=sampler):
        step = sampler.step                          # the sampler continues its sequence where the saved run stopped
    while step < a.steps:
        n = min(a.print_steps, a.steps - step)
        loss = teacher.fit(sampler, n)[-1]
        step += n
        x = data.audio[sampler.indices.long(), :a.num_samples].cpu().numpy()      # the last batch drawn ("head" crop)
        regen = teacher.reconstruct(x, None); enc = teacher.encode(x, None)
        print(step - 1, float(loss), "reconstruction rms %.3f" % float(np.sqrt(np.mean(regen ** 2))), "encoding", enc.shape, flush=True)
        if teacher.save(a.teacher, step - 1, force=False) and a.resume:
            teacher.save_training_state(a.teacher, step - 1, sampler=sampler)
    teacher.save(a.teacher, a.steps - 1, force=True)
    if a.resume:
        teacher.save_training_state(a.teacher, a.steps - 1, sampler=sampler)
    return None if loss is None else float(loss)


if __name__ == "__main__":
    main()
