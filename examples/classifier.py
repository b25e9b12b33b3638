#!/usr/bin/env python3
"""Parallel driver to the reference's ``train.py --classifier`` / ``--test``: the same ``WaveNet`` call (two blocks of
dilations 1..512, 32 / 128 channels, learning rate 1e-3) on generated waves labelled by wave shape, the way
examples/siamese.py labels them; no TensorFlow session, no recordings on disk.

  python examples/classifier.py --train --logdir runs/classifier --steps 1000
  python examples/classifier.py --test --logdir runs/classifier
  python examples/classifier.py --train --test --logdir runs/classifier --steps 1000 --device-data

Without ``--device-data`` this is train.py's host loop: ``train(x, y)`` per batch, ``predict(x)`` per test clip.  With it
the training set and the test set are loaded onto the device once: the steps between two prints are one ``fit`` call that
also sweeps a validation set every ``--validate-every`` steps (``fit(..., validate=...)``), and ``--test`` is one
``evaluate`` call.  ``--shift``, ``--gain``, ``--noise``, ``--noise-prob`` and ``--noise-volume`` augment the training draws
there (``dataset.Augment``), and ``--speed LO:HI`` (with ``--resample-taps``) resamples every drawn clip by a random factor,
tempo and pitch together; ``--rir FILE.npy`` with ``--rir-prob P`` convolves a drawn clip with one of the file's room
impulse responses (``dataset.prepare_rirs``, ``dataset.synthetic_rirs``).  The validation and test sets are never
augmented."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-wavenet_amd", "dropin"))
import numpy as np                                   # noqa: E402
from model import WaveNet                            # noqa: E402
from simple_audio import generate_random_wave        # noqa: E402

WORDS = ["wave%d" % i for i in range(4)]             # (the reference's idxToLabel: the four wave shapes)


def make_set(count, num_samples, rng):
    waves = [generate_random_wave(num_samples, rng=rng) for _ in range(count)]
    return (np.array([w for w, _ in waves], dtype=np.float32), np.array([int(np.argmax(y)) for _, y in waves]))


def report(correct, total):
    """train.py:117-121 from per-class (correct, total) counts."""
    correct_count, all_count = int(np.sum(correct)), int(np.sum(total))
    print("Correct: {:d} | Wrong: {:d} | Total: {:d} | % Correct: {:.3f}".format(
        correct_count, all_count - correct_count, all_count, correct_count / float(max(all_count, 1))), flush=True)
    print("Correct", {w: int(c) for w, c, t in zip(WORDS, correct, total) if t}, flush=True)
    print("Wrongs", {w: int(t - c) for w, c, t in zip(WORDS, correct, total) if t}, flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--logdir", type=str, default="events/%d" % int(time.time() * 1000),
                   help="directory where checkpoints are stored")
    p.add_argument("--train", action="store_true", help="train the classifier")
    p.add_argument("--test", action="store_true", help="sweep the test set once and print the counts")
    p.add_argument("--steps", type=int, default=100000)
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--num-samples", type=int, default=16384)
    p.add_argument("--print-steps", type=int, default=100)
    p.add_argument("--seed", type=int, default=None, help="seed of the wave generator (default: unseeded)")
    p.add_argument("--layers", type=int, default=20)
    p.add_argument("--test-clips", type=int, default=200)
    p.add_argument("--device-data", action="store_true",
                   help="hold the training, validation and test sets on the device (model.fit / model.evaluate)")
    p.add_argument("--device-clips", type=int, default=256, help="--device-data: generated waves in the training set")
    p.add_argument("--validation-clips", type=int, default=64)
    p.add_argument("--validate-every", type=int, default=100, help="--device-data: training steps between two sweeps")
    p.add_argument("--eval-batch-size", type=int, default=8)
    import importlib
    O = importlib.import_module("sr-wavenet_amd.optim")
    O.add_control_flags(p, validate=True)
    DS = importlib.import_module("sr-wavenet_amd.dataset")
    DS.add_augment_flags(p)
    a = p.parse_args(argv)
    a.augment = DS.augment_from_flags(a, a.device_data)         # (refuses the flags without --device-data)
    rng = np.random.RandomState(a.seed) if a.seed is not None else None
    num_classes = len(WORDS)
    dilations = ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2)[:a.layers]
    network = WaveNet(a.num_samples, num_classes, dilations, dilation_channels=32, skip_channels=128,
                      output_channels=num_classes, learning_rate=0.001)                     # train.py:39
    if a.train:
        O.apply_control_flags(network, a, 0.001, a.steps)
    network.load(a.logdir)
    D = None
    if a.device_data:
        D = importlib.import_module("sr-wavenet_amd.dataset")
    if a.train and a.device_data:
        fit_loop(a, network, D, rng)
    elif a.train:
        global_step = first = network.training_step() if a.resume and network.load_training_state(a.logdir) else 0
        for global_step in range(first, a.steps):
            x, labels = make_set(a.batch_size, a.num_samples, rng)
            y = np.eye(num_classes, dtype=np.float32)[labels]
            loss = network.train(x, y)
            if global_step % a.print_steps == 0:
                probs = network.predict(x)[:, 0, :]
                print("Step: {:6d} | Loss: {:.4f} | Correct Pred: {:.4f} | Real: {} | Predicted: {}".format(
                    global_step, loss, np.sum(y * probs), WORDS[labels[0]], WORDS[int(np.argmax(probs[0]))]), flush=True)
            if network.save(a.logdir, global_step, force=False) and a.resume:             # once per minute
                network.save_training_state(a.logdir, global_step)
        network.save(a.logdir, global_step, force=True)
        if a.resume:
            network.save_training_state(a.logdir, global_step)
    if a.test:
        x, labels = make_set(a.test_clips, a.num_samples, rng)
        if a.device_data:
            data = D.DeviceDataset(x, labels, num_classes)
            result = network.evaluate(data.eval_sampler(a.eval_batch_size, a.num_samples))
            correct, total = result.per_class[:, 0], result.per_class[:, 1]
        else:
            correct, total = np.zeros(num_classes, np.int64), np.zeros(num_classes, np.int64)
            for clip, label in zip(x, labels):                                              # train.py:94-115
                probs = network.predict(np.array([clip]))
                total[label] += 1
                correct[label] += int(np.argmax(probs) == label)
        report(correct, total)
        return int(np.sum(correct)), int(np.sum(total))
    return None


def fit_loop(a, network, D, rng):
    """--device-data: the training and validation sets are loaded onto the device once; the steps between two prints are
    one ``fit`` call, and every ``--validate-every`` steps a sweep of the validation set rides along without a host wait
    of its own."""
    train = D.DeviceDataset(*make_set(a.device_clips, a.num_samples, rng), len(WORDS))
    held = D.DeviceDataset(*make_set(a.validation_clips, a.num_samples, rng), len(WORDS))
    sampler = train.sampler(a.batch_size, a.num_samples, seed=0, augment=a.augment)     # (the held-out sets stay plain)
    validation = held.eval_sampler(a.eval_batch_size, a.num_samples)
    print("%d + %d clips of %d samples on the device (%.1f MB)" % (len(train), len(held), train.clip_len,
                                                                  (train.nbytes + held.nbytes) / 1e6), flush=True)
    step = 0
    if a.resume and network.load_training_state(a.logdir, sampler=sampler):
        step = sampler.step                          # the sampler continues its sequence where the saved run stopped
    first = step
    while step < a.steps:
        n = min(a.print_steps, a.steps - step)
        losses, sweeps = network.fit(sampler, n, validate=(validation, a.validate_every))
        step += n
        print("Step: {:6d} | Loss: {:.4f}".format(step - 1, losses[-1]), flush=True)
        for r in sweeps:
            print("Step: {:6d} | Validation: {:d} of {:d} | % Correct: {:.3f} | NLL: {:.4f}".format(
                r.step, int(np.trace(r.confusion)), r.seen, r.accuracy, r.mean_nll), flush=True)
        if network.save(a.logdir, step - 1, force=False) and a.resume:
            network.save_training_state(a.logdir, step - 1, sampler=sampler)
    if step > first or (step and not a.resume):
        network.save(a.logdir, step - 1, force=True)
        if a.resume:
            network.save_training_state(a.logdir, step - 1, sampler=sampler)


if __name__ == "__main__":
    main()
