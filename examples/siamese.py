#!/usr/bin/env python3
"""Parallel driver to the reference's siamese.py: random wave pairs, label 1 when both clips use the same wave shapes,
``SiameseWaveNet.train``; same model calls, no TensorFlow session, no plotting.  ``--test`` prints embeddings; with
``--device-data`` it sweeps a labelled held-out set on the device and prints what a verification model is judged by.

  python examples/siamese.py --train --logdir runs/siamese --steps 1000
  python examples/siamese.py --test --logdir runs/siamese
  python examples/siamese.py --train --logdir runs/siamese --steps 1000 --device-data
  python examples/siamese.py --test --logdir runs/siamese --device-data --test-clips 1024
  python examples/siamese.py --train --logdir runs/siamese --steps 1000 --device-data --shift 100 --gain 0.7:1.3

``--shift``, ``--gain``, ``--noise``, ``--noise-prob`` and ``--noise-volume`` augment the pairs drawn with ``--device-data``
(``dataset.Augment``): the two clips of a pair independently, so two views of one recording differ.  ``--speed LO:HI``
(with ``--resample-taps``) resamples each clip by a random factor of its own, tempo and pitch together.
``--rir FILE.npy`` with ``--rir-prob P`` reverberates each clip with a room impulse response of its own: two views of one
recording then differ the way two rooms do.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-wavenet_amd", "dropin"))
import numpy as np                                   # noqa: E402
from model import SiameseWaveNet                     # noqa: E402
from simple_audio import generate_random_wave        # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--logdir", type=str, default="siamese/%d" % int(time.time() * 1000),
                   help="directory where checkpoints are stored")
    p.add_argument("--start", type=int, default=0, help="starting step")
    p.add_argument("--train", action="store_true", help="train the siamese network")
    p.add_argument("--test", action="store_true", help="print embeddings of random wave pairs")
    p.add_argument("--steps", type=int, default=1000000, help="last training step (exclusive)")
    p.add_argument("--batch-size", type=int, default=1, help="pairs per step")
    p.add_argument("--num-samples", type=int, default=5120)
    p.add_argument("--print-steps", type=int, default=100)
    p.add_argument("--seed", type=int, default=None, help="seed of the wave generator (default: unseeded)")
    p.add_argument("--layers", type=int, default=30)
    p.add_argument("--device-data", action="store_true",
                   help="--train on pairs drawn on the device from a labelled set held there (model.fit)")
    p.add_argument("--tfrecord", type=str, default=None, help="--device-data: an NSynth TFRecord file, labelled by --label-key")
    p.add_argument("--audio-max-length", type=int, default=16000)
    p.add_argument("--label-key", type=str, default="instrument_family")
    p.add_argument("--num-classes", type=int, default=11)
    p.add_argument("--device-clips", type=int, default=256,
                   help="--device-data without --tfrecord: generated waves to hold, labelled by wave shape")
    p.add_argument("--test-clips", type=int, default=256,
                   help="--test --device-data without --tfrecord: generated waves of the held-out set")
    p.add_argument("--eval-batch-size", type=int, default=8, help="--test --device-data: clips per step of the sweep")
    p.add_argument("--bins", type=int, default=512, help="--test --device-data: bins of the distance histograms")
    import importlib
    O = importlib.import_module("sr-wavenet_amd.optim")
    O.add_control_flags(p)
    DS = importlib.import_module("sr-wavenet_amd.dataset")
    DS.add_augment_flags(p)
    a = p.parse_args(argv)
    a.augment = DS.augment_from_flags(a, a.device_data)         # (refuses the flags without --device-data)
    rng = np.random.RandomState(a.seed) if a.seed is not None else None
    dilations = ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3)[:a.layers]
    network = SiameseWaveNet(input_size=a.num_samples, output_dimensions=2, dilations=dilations, skip_channels=128,
                             learning_rate=1e-4)                                             # siamese.py:44
    sess = None                                                                               # accepted and ignored
    if a.train:
        O.apply_control_flags(network, a, 1e-4, a.steps)
    network.load(sess, a.logdir)
    loss = None
    if a.train and a.device_data:
        loss = fit_loop(a, network, rng)
    elif a.train:
        if a.resume and network.load_training_state(a.logdir):
            a.start = network.training_step()
        global_step = a.start
        for global_step in range(a.start, a.steps):
            pairs = [(generate_random_wave(a.num_samples, rng=rng), generate_random_wave(a.num_samples, rng=rng))
                     for _ in range(a.batch_size)]
            x1 = np.array([w1 for (w1, _), _ in pairs], dtype=np.float32)
            x2 = np.array([w2 for _, (w2, _) in pairs], dtype=np.float32)
            labels = np.array([(y1 == y2).all() for (_, y1), (_, y2) in pairs], dtype=np.float32)
            loss, distance = network.train(sess, x1, x2, labels)
            if global_step % a.print_steps == 0:
                print(global_step, loss, distance, labels, flush=True)
            if network.save(sess, a.logdir, global_step, force=False) and a.resume:        # once per minute
                network.save_training_state(a.logdir, global_step)
        network.save(sess, a.logdir, global_step, force=True)
        if a.resume:
            network.save_training_state(a.logdir, global_step)
    if a.test and a.device_data:
        test_sweep(a, network, rng)
    elif a.test:
        for _ in range(10):
            x1, y1 = generate_random_wave(a.num_samples, rng=rng)
            x2, y2 = generate_random_wave(a.num_samples, rng=rng)
            embedding1 = network.get_embedding(sess, [x1, x2])
            embedding2 = network.get_embedding(sess, [x2])
            print(embedding1, embedding2, (y1 == y2).all(), embedding1.shape, flush=True)
    return None if loss is None else float(loss)


def labelled_set(a, clips, rng, limit=None):
    """The TFRecord file with its --label-key feature, or `clips` generated waves labelled by wave shape, on the device."""
    import importlib
    D = importlib.import_module("sr-wavenet_amd.dataset")
    if a.tfrecord:
        return D.DeviceDataset.from_tfrecord(a.tfrecord, a.audio_max_length, label_key=a.label_key,
                                             num_classes=a.num_classes, limit=limit)
    waves = [generate_random_wave(a.num_samples, rng=rng) for _ in range(clips)]
    return D.DeviceDataset(np.array([w for w, _ in waves], dtype=np.float32),
                           np.array([int(np.argmax(y)) for _, y in waves]), 4)


def test_sweep(a, network, rng):
    """--test --device-data: one sweep of a labelled held-out set through a tower and one launch over all its pairs
    (``SiameseWaveNet.evaluate``): nearest-neighbour accuracy, recall@k, equal error rate, AUC."""
    import importlib
    D = importlib.import_module("sr-wavenet_amd.dataset")
    data = labelled_set(a, a.test_clips, rng, limit=D.MAX_EMBED_RECORDS)
    res = network.evaluate(data.embed_sampler(a.eval_batch_size, a.num_samples, bins=a.bins))
    far, frr = res.far_frr(res.eer_threshold) if np.isfinite(res.eer_threshold) else (float("nan"), float("nan"))
    print("Held-out: %d clips | pairs: %d same, %d different" % (res.seen, res.hist_same.sum(), res.hist_diff.sum()))
    print("1-NN accuracy: %.4f | recall@5: %.4f | recall@10: %.4f" % (res.nn_accuracy, res.recall_at(5), res.recall_at(10)))
    print("EER: %.4f at distance %.4f (FAR %.4f, FRR %.4f) | AUC: %.4f" % (res.eer, res.eer_threshold, far, frr, res.auc),
          flush=True)
    return res


def fit_loop(a, network, rng):
    """--device-data: a labelled set of recordings -- the TFRecord file with its --label-key feature, or a fixed set of
    generated waves labelled by wave shape -- is loaded onto the device once; every step draws its pairs there ("same
    class" for half of them) and the steps between two prints are one ``fit`` call."""
    data = labelled_set(a, a.device_clips, rng)
    sampler = data.pair_sampler(a.batch_size, a.num_samples, seed=0, augment=a.augment)   # (two views of a pair differ)
    sampler.seek(a.start)
    if a.resume and network.load_training_state(a.logdir, sampler=sampler):
        a.start = sampler.step                       # the sampler continues its sequence where the saved run stopped
    print("%d clips of %d samples on the device (%.1f MB)" % (len(data), data.clip_len, data.nbytes / 1e6), flush=True)
    loss, step = None, a.start
    while step < a.steps:
        n = min(a.print_steps, a.steps - step)
        losses, distance = network.fit(sampler, n)
        step += n
        loss = losses[-1]
        print(step - 1, loss, distance[-1], sampler.y.cpu().numpy(), flush=True)
        if network.save(None, a.logdir, step - 1, force=False) and a.resume:
            network.save_training_state(a.logdir, step - 1, sampler=sampler)
    if loss is not None:
        network.save(None, a.logdir, step - 1, force=True)
        if a.resume:
            network.save_training_state(a.logdir, step - 1, sampler=sampler)
    return loss


if __name__ == "__main__":
    main()
