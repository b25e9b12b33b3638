#!/usr/bin/env python3
"""Parallel driver to the reference's siamese.py: random wave pairs, label 1 when both clips use the same wave shapes,
``SiameseWaveNet.train``; same model calls, no TensorFlow session, no plotting.  ``--test`` prints embeddings.

  python examples/siamese.py --train --logdir runs/siamese --steps 1000
  python examples/siamese.py --test --logdir runs/siamese
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
    a = p.parse_args(argv)
    rng = np.random.RandomState(a.seed) if a.seed is not None else None
    dilations = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
    network = SiameseWaveNet(input_size=a.num_samples, output_dimensions=2, dilations=dilations, skip_channels=128,
                             learning_rate=1e-4)                                             # siamese.py:44
    sess = None                                                                               # accepted and ignored
    network.load(sess, a.logdir)
    loss = None
    if a.train:
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
            network.save(sess, a.logdir, global_step, force=False)                         # once per minute
        network.save(sess, a.logdir, global_step, force=True)
    if a.test:
        for _ in range(10):
            x1, y1 = generate_random_wave(a.num_samples, rng=rng)
            x2, y2 = generate_random_wave(a.num_samples, rng=rng)
            embedding1 = network.get_embedding(sess, [x1, x2])
            embedding2 = network.get_embedding(sess, [x2])
            print(embedding1, embedding2, (y1 == y2).all(), embedding1.shape, flush=True)
    return None if loss is None else float(loss)


if __name__ == "__main__":
    main()
