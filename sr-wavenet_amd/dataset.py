"""Device-resident datasets: the clips stay on the MI355X and every batch is drawn inside the training step.

``DeviceDataset`` holds ``[N, clip_len]`` fp32 clips (and int32 labels) in device memory; ``dataset.sampler(...)`` returns
a ``BatchSampler`` whose two launches (csrc/srwn_data.hip) ride in the step's hipGraph: ``srwn_batch_draw`` in front -- it
reads the step counter from device memory, picks the batch's records and crop offsets and writes everything the engines'
``set_inputs`` writes from a host batch -- and ``srwn_step_log`` behind, which stores the step's loss in a ring and ticks
the counter.  ``fit(sampler, steps)`` on the model classes (model.py) is then ``steps`` graph replays with no upload and
one host wait per call.

The order of the samples is a pure function of ``(seed, step, b, rank, world, N)``; ``draw_plan`` below states it in
Python and is its specification, the kernel implements it.  Repetition comes before batching, so batches run across epoch
boundaries (nsynth.py:39-45), and every epoch is a fresh keyed permutation of the records.  The reference's shuffle
buffer of 10 000 records is NOT reproduced: TensorFlow's shuffle order is not reproducible either (see nsynth.py's
docstring), and a permutation of the whole set is the stronger shuffle.

Two more samplers feed the models whose step needs more than clips (csrc/srwn_draw.hip): a ``DistillSampler`` draws the
student's clips, its logistic noise (``noise_plan``) and the labels' one-hot rows into every conditioning input, and logs
loss, power loss and entropy; a ``PairSampler`` draws "same class" / "different class" pairs of a labelled set
(``pair_plan``) for the twin towers and logs the loss and the pairs' distances.

Held-out evaluation runs the same way (csrc/srwn_eval.hip): an ``EvalSampler`` sweeps a labelled set once, in order
(``sweep_plan``: the last step may be ragged), its draw is ``srwn_batch_draw`` and the launch behind the forward pass,
``srwn_eval_classes``, turns the step's posteriors into predicted classes, ranks, per-clip NLL and confusion counts in one
of ``sweep_capacity`` result slots on the device and ticks the state ``{seed, step, sweep}``; ``WaveNet.evaluate`` and
``WaveNet.fit(..., validate=...)`` (model.py) read the slots into ``EvalResult``s.

An embedding model is judged over all pairs of the held-out set (csrc/srwn_pair_eval.hip): an ``EmbedSampler`` sweeps the
set the same way, ``srwn_embed_collect`` behind the tower's forward pass gathers the embeddings in a result slot, and one
``srwn_pair_sweep`` behind the sweep's last step turns the slot's N x N distances into nearest neighbours, the rank of the
nearest record of the same label and the two distance histograms; ``SiameseWaveNet.evaluate`` and ``SiameseWaveNet.fit(...,
validate=...)`` read the slots into ``PairEvalResult``s (nearest-neighbour accuracy, recall@k, FAR / FRR, EER, AUC).

A ``BatchSampler`` or a ``PairSampler`` built with ``augment=Augment(...)`` draws augmented rows (csrc/srwn_augment.hip):
a random time shift with zero fill, a random gain and a background clip of another ``DeviceDataset`` mixed in at a random
volume, per row and per step, in the draw launch itself.  ``augment_plan`` states the row's draws and ``augment_rows`` the
sample rule; the kernels give their bits.  A ``PairSampler`` augments the two clips of a pair as two sides of one position,
so two views of one record differ.  Evaluation sweeps are not augmented.

``Augment(speed=(lo, hi))`` adds speed perturbation in front of that rule (csrc/srwn_resample.hip): every row is resampled
by a factor of its own near 1, ``y(j) = x(j * s)``, through a windowed-sinc polyphase table -- tempo and pitch move
together, by ``12 log2(s)`` semitones.  ``speed_plan`` states the row's fixed-point step, ``resample_table`` the filter and
``resample_rows`` the sample rule; shift, gain, noise and clamp then act on the resampled row.

Storage is fp32 only: int16 or bf16 clip storage is out of scope.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import numpy as np

_MASK = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_CROP_SALT = 0x63726F706F666673
NOISE_SALT = 0x6E6F697365726F77        # the rows' noise seeds
PAIR_SALT = 0x70616972636F696E         # the pairs' coins ...
PAIR_PICK_SALT = 0x706169727069636B    # ... their right records
PAIR_CROP_SALT = 0x7061697263726F70    # ... and the right clips' crop offsets
AUG_SHIFT_SALT = 0x6175677368696674     # an augmented row's shift ...
AUG_GAIN_SALT = 0x6175676761696E21      # ... its gain
AUG_COIN_SALT = 0x617567636F696E21      # ... whether noise is mixed in
AUG_PICK_SALT = 0x6175677069636B21      # ... the noise record
AUG_OFFSET_SALT = 0x6175676F66667374    # ... where its window starts
AUG_VOLUME_SALT = 0x617567766F6C2121    # ... and its volume
AUG_SPEED_SALT = 0x6175677370656564     # ... and the step it is resampled at
AUG_RIR_COIN_SALT = 0x61756772636F696E  # ... whether it is reverberated ("augrcoin")
AUG_RIR_PICK_SALT = 0x617567727069636B  # ... and with which room response ("augrpick")
SPEED_BITS = 24            # a speed is a fixed-point step with this many fraction bits: step = round(s * 2^24)
SPEED_ONE = 1 << SPEED_BITS
RESAMPLE_PHASES = 4096     # phases of the polyphase table (SRWN_RESAMPLE_PHASES in srwn.h); a power of two
RESAMPLE_BETA = 7.0        # its Kaiser window (DESIGN section 5f says why these two)
ROOM_MAX_TAPS = 8192       # taps of a room impulse response (SRWN_ROOM_MAX_TAPS in srwn.h): 0.51 s at 16 kHz
_ROUNDS = 4
CROPS = {"head": 0, "random": 1}
MAX_BATCH = 65535          # rows of one draw (the launch's second grid dimension)


def _mix64(x: int) -> int:
    """The splitmix64 finaliser (the one the generators' ``gen_uniform`` keys its draws with)."""
    x &= _MASK
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _MASK
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _MASK
    x ^= x >> 31
    return x


def permute(seed: int, epoch: int, i: int, n: int) -> int:
    """perm(seed, epoch)(i): a keyed bijection on [0, n).  Four alternating Feistel rounds on the k = ceil(log2 n) bits
    of the next power of two (halves of k // 2 and k - k // 2 bits that swap widths every round), cycle-walked until the
    value is back in [0, n): the walk follows one cycle of a permutation of 2^k points, so it ends within 2^k steps."""
    if n <= 1:
        return 0
    k = (n - 1).bit_length()
    ekey = _mix64(seed + _GOLDEN * (epoch + 1))
    x = i
    for _ in range(1 << k):
        a, b = k // 2, k - k // 2
        for r in range(_ROUNDS):
            left, right = x >> b, x & ((1 << b) - 1)
            f = _mix64(ekey + _GOLDEN * (right * _ROUNDS + r + 1)) & 0xFFFFFFFF
            x = (right << a) | (left ^ (f & ((1 << a) - 1)))
            a, b = b, a
        if x < n:
            return x
    raise AssertionError("cycle walk left its cycle")       # (a bijection cannot)


def draw_plan(seed: int, step: int, batch_size: int, n: int, clip_len: int, num_samples: int, shuffle: bool = True,
              crop: str = "head", rank: int = 0, world: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The batch of ``step``: ``(indices [B] int32, offsets [B] int64)``.  Row b is position
    p = (step * world + rank) * B + b of the sample sequence: epoch e = p // n, place i = p % n, record
    ``permute(seed, e, i, n)`` with ``shuffle`` and ``i`` without; the crop starts at 0 ("head": tf.slice, nsynth.py:31)
    or at an offset uniform on [0, clip_len - num_samples] keyed by (seed, p) ("random")."""
    _check_draw(batch_size, n, clip_len, num_samples, crop, rank, world)
    seed &= _MASK
    idx = np.empty(batch_size, np.int32)
    off = np.zeros(batch_size, np.int64)
    for b in range(batch_size):
        p = (step * world + rank) * batch_size + b
        e, i = divmod(p, n)
        idx[b] = permute(seed, e, i, n) if shuffle else i
        if CROPS[crop]:
            h = _mix64((seed ^ _CROP_SALT) + _GOLDEN * (p + 1))
            off[b] = ((h >> 32) * (clip_len - num_samples + 1)) >> 32
    return idx, off


def sweep_steps(n: int, batch_size: int, world: int = 1) -> int:
    """The steps of one sweep over `n` records: ceil(n / (batch_size * world))."""
    n, batch_size, world = int(n), int(batch_size), int(world)
    if n < 1:
        raise ValueError("the dataset is empty")
    if batch_size < 1 or world < 1:
        raise ValueError("sweep_steps: batch_size %d, world %d" % (batch_size, world))
    return -(-n // (batch_size * world))


def sweep_plan(step: int, batch_size: int, n: int, rank: int = 0, world: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The batch of step `step` of a sweep that visits every record once: ``(indices [B] int32, valid [B] bool)``.  Row b is
    position p = (step * world + rank) * B + b; it is valid where p < n and its record is p % n -- ``draw_plan``'s record
    without shuffling, so ``srwn_batch_draw`` is the sweep's draw and the rows of the ragged tail read inside the set.
    ``sweep_steps(n, B, world)`` steps of all ranks hold every record exactly once among their valid rows."""
    step, batch_size, n, rank, world = int(step), int(batch_size), int(n), int(rank), int(world)
    if n < 1:
        raise ValueError("the dataset is empty")
    if not 1 <= batch_size <= MAX_BATCH:
        raise ValueError("batch_size %d: at least 1, at most %d" % (batch_size, MAX_BATCH))
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of %d" % (rank, world))
    if step < 0:
        raise ValueError("step %d" % step)
    p = (step * world + rank) * batch_size + np.arange(batch_size, dtype=np.int64)
    return (p % n).astype(np.int32), p < n


def noise_rows(seed: int, step: int, batch_size: int, rank: int = 0, world: int = 1) -> np.ndarray:
    """The seeds s_b of the step's noise rows, uint64 [B]: ``_mix64((seed ^ NOISE_SALT) + _GOLDEN * (p + 1))`` at the
    row's position p = (step * world + rank) * B + b."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of %d" % (rank, world))
    seed &= _MASK
    return np.array([_mix64((seed ^ NOISE_SALT) + _GOLDEN * ((step * world + rank) * batch_size + b + 1))
                     for b in range(batch_size)], dtype=np.uint64)


def noise_plan(seed: int, step: int, batch_size: int, num_samples: int, rank: int = 0, world: int = 1) -> np.ndarray:
    """The 23-bit values k of the step's logistic noise, uint32 [B, T]: ``k[b, j] = _mix64(s_b + _GOLDEN * (j + 1)) >> 41``
    with the row seeds of ``noise_rows`` -- what ``srwn_logistic_noise`` draws for ``seed[b] = s_b`` at clock 0.  The
    noise is ``temperature * (log u - log(1 - u))`` at ``u = (k + 1/2) / 2^23``, by that kernel's own evaluation
    (``srwn_logistic_from_bits``)."""
    if batch_size < 1 or num_samples < 1:
        raise ValueError("noise_plan: batch_size %d, num_samples %d" % (batch_size, num_samples))
    rows = noise_rows(seed, step, batch_size, rank, world)
    # splitmix64 over whole rows in uint64 arithmetic (wraps as the masks of _mix64 do)
    j = np.arange(1, num_samples + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = rows[:, None] + np.uint64(_GOLDEN) * j[None, :]
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(41)).astype(np.uint32)


def class_index(labels, num_classes: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(order [N] int32, place [N] int32, start [num_classes + 1] int32)``: the stable argsort of the labels, its inverse
    and where each class begins in it.  Every label must lie in [0, num_classes)."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    if int(num_classes) < 1:
        raise ValueError("num_classes %d: at least 1" % int(num_classes))
    if lab.size < 1:
        raise ValueError("the dataset is empty")
    if lab.min() < 0 or lab.max() >= int(num_classes):
        raise ValueError("pairs need every label inside [0, %d); got labels from %d to %d"
                         % (int(num_classes), int(lab.min()), int(lab.max())))
    order = np.argsort(lab, kind="stable").astype(np.int32)
    place = np.empty_like(order)
    place[order] = np.arange(lab.size, dtype=np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=int(num_classes)))]).astype(np.int32)
    return order, place, start


def same_threshold(p_same: float) -> int:
    """floor(p_same * 2^32): the coin of a pair says "same" where its 32 bits lie below it."""
    if not 0.0 <= float(p_same) <= 1.0:
        raise ValueError("p_same %r: a probability" % (p_same,))
    return int(float(p_same) * 4294967296.0)


def pair_plan(seed: int, step: int, pairs: int, labels, num_classes: int, clip_len: int, num_samples: int,
              p_same: float = 0.5, shuffle: bool = True, crop: str = "head", rank: int = 0, world: int = 1):
    """The pairs of ``step``: ``(left [P] int32, right [P] int32, off_left [P] int64, off_right [P] int64, y [P]
    float32)``.  The left side is ``draw_plan``'s record and offset of position p = (step * world + rank) * P + b.  With c
    its label, m the records of class c, N all records and q the left record's place inside its class block of the stable
    argsort ``order`` of the labels: the coin ``same = (h1 >> 32) < floor(p_same * 2^32)`` is overridden where only one
    outcome exists (m == 1: different; N == m: same; N == 1: the record with itself).  Same: ``k = ((h2 >> 32) * (m - 1))
    >> 32``, ``k += (k >= q)`` (never the clip itself), right = ``order[start[c] + k]``.  Different: ``k = ((h2 >> 32) *
    (N - m)) >> 32``, right = ``order[k if k < start[c] else k + m]``.  h1, h2 and (crop "random") the right offset's h3
    are ``_mix64((seed ^ salt) + _GOLDEN * (p + 1))`` with PAIR_SALT, PAIR_PICK_SALT and PAIR_CROP_SALT; the offset
    follows ``draw_plan``'s formula.  y = 1.0 where the labels agree, else 0.0 (the reference's convention,
    model.py:747-749)."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    order, place, start = class_index(lab, num_classes)
    n = int(lab.size)
    left, off_left = draw_plan(seed, step, pairs, n, clip_len, num_samples, shuffle, crop, rank, world)
    thr = same_threshold(p_same)
    seed &= _MASK
    right = np.empty(pairs, np.int32)
    off_right = np.zeros(pairs, np.int64)
    for b in range(pairs):
        p = (step * world + rank) * pairs + b
        rec = int(left[b])
        c = int(lab[rec])
        s0 = int(start[c])
        m = int(start[c + 1]) - s0
        q = int(place[rec]) - s0
        h1 = _mix64((seed ^ PAIR_SALT) + _GOLDEN * (p + 1))
        h2 = _mix64((seed ^ PAIR_PICK_SALT) + _GOLDEN * (p + 1)) >> 32
        same = (h1 >> 32) < thr
        if m == 1:
            same = False
        if n == m:
            same = True
        if n == 1:
            right[b] = rec
        elif same:
            k = (h2 * (m - 1)) >> 32
            k += k >= q
            right[b] = order[s0 + k]
        else:
            k = (h2 * (n - m)) >> 32
            right[b] = order[k if k < s0 else k + m]
        if CROPS[crop]:
            h3 = _mix64((seed ^ PAIR_CROP_SALT) + _GOLDEN * (p + 1))
            off_right[b] = ((h3 >> 32) * (clip_len - num_samples + 1)) >> 32
    y = (lab[left] == lab[right]).astype(np.float32)
    return left, right, off_left, off_right, y


def _check_draw(batch_size, n, clip_len, num_samples, crop, rank, world):
    if crop not in CROPS:
        raise ValueError("crop %r: 'head' or 'random'" % (crop,))
    if n < 1:
        raise ValueError("the dataset is empty")
    if not 1 <= batch_size <= MAX_BATCH:
        raise ValueError("batch_size %d: at least 1, at most %d" % (batch_size, MAX_BATCH))
    if num_samples < 1:
        raise ValueError("num_samples %d: at least 1" % num_samples)
    if num_samples > clip_len:
        raise ValueError("num_samples %d > clip length %d (tf.slice would fail, nsynth.py:31)" % (num_samples, clip_len))
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of %d" % (rank, world))


class DeviceDataset(object):
    """``audio [N, clip_len]`` float32 and optional integer ``labels [N]`` (classes ``[0, num_classes)``) held on the
    device as fp32 and int32 -- the only storage formats: int16 / bf16 clips are out of scope."""

    def __init__(self, audio, labels=None, num_classes: int = 0, device="cuda"):
        a = np.asarray(audio) if not _is_tensor(audio) else audio
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("audio must be [clips, samples], got %s" % (tuple(a.shape),))
        if a.shape[0] >= 1 << 31:
            raise ValueError("at most 2^31 - 1 clips")
        n = int(a.shape[0])
        lab = None
        if labels is not None:
            lab = np.asarray(labels) if not _is_tensor(labels) else labels.detach().cpu().numpy()
            if lab.shape != (n,):
                raise ValueError("labels must be [%d], got %s" % (n, tuple(lab.shape)))
            if lab.dtype.kind not in "iu":
                raise TypeError("labels must be integers, got %s" % lab.dtype)
            if int(num_classes) < 1:
                raise ValueError("labels need num_classes >= 1 (the width of their one-hot rows)")
            lab = np.clip(lab.astype(np.int64), -1, int(num_classes)).astype(np.int32)   # outside the classes either way
        elif int(num_classes):
            raise ValueError("num_classes without labels")
        import torch
        from . import kernels as K
        K._need_gpu()
        self.device = torch.device(device)
        if _is_tensor(a):
            self.audio = a.detach().to(device=self.device, dtype=torch.float32).contiguous()
        else:
            self.audio = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.labels = None if lab is None else torch.as_tensor(lab).to(self.device)
        self.num_classes = int(num_classes)

    @classmethod
    def from_tfrecord(cls, path, audio_max_length, label_key="pitch", num_classes=128, limit=None, device="cuda",
                      piece: int = 256):
        """The clips (all `audio_max_length` samples of each) and the `label_key` feature of an NSynth TFRecord file,
        read through ``nsynth.TFRecordFile.batch`` in pieces of `piece` records and uploaded piece by piece."""
        import torch
        from . import kernels as K
        from .nsynth import TFRecordFile
        K._need_gpu()
        f = TFRecordFile(path)
        try:
            n = len(f) if limit is None else min(len(f), int(limit))
            if n < 1:
                raise ValueError("%s holds no records" % path)
            audio = torch.empty((n, int(audio_max_length)), dtype=torch.float32, device=device)
            labels = np.empty(n, np.int64)
            for i0 in range(0, n, int(piece)):
                i1 = min(n, i0 + int(piece))
                a, lab = f.batch(np.arange(i0, i1), int(audio_max_length), int(audio_max_length), label_key)
                audio[i0:i1].copy_(torch.from_numpy(a))
                labels[i0:i1] = lab
        finally:
            f.close()
        return cls(audio, labels if label_key else None, num_classes if label_key else 0, device)

    def __len__(self):
        return int(self.audio.shape[0])

    @property
    def clip_len(self) -> int:
        return int(self.audio.shape[1])

    @property
    def nbytes(self) -> int:
        """Device bytes of the clips and the labels."""
        return self.audio.numel() * 4 + (0 if self.labels is None else self.labels.numel() * 4)

    def sampler(self, batch_size, num_samples, seed=0, shuffle=True, crop="head", rank=0, world=1, log_capacity=1024,
                augment=None):
        """The draws of a training run (``fit`` of the classifier, the teacher, the auto-encoder); with `augment` (an
        ``Augment``) every drawn row is shifted, scaled and mixed with noise in the draw launch."""
        return BatchSampler(self, batch_size, num_samples, seed, shuffle, crop, rank, world, log_capacity, augment)

    def distill_sampler(self, batch_size, num_samples, seed=0, shuffle=True, crop="head", temperature=1.0, rank=0, world=1,
                        log_capacity=1024):
        """The draws of a student's distillation run (``ParallelWaveNet.fit``): clips, logistic noise, one-hot rows."""
        return DistillSampler(self, batch_size, num_samples, seed, shuffle, crop, temperature, rank, world, log_capacity)

    def pair_sampler(self, pairs, num_samples, seed=0, p_same=0.5, shuffle=True, crop="head", rank=0, world=1,
                     log_capacity=1024, augment=None):
        """The draws of a twin-tower run (``SiameseWaveNet.fit``): `pairs` pairs of clips per step, "same class" with
        probability `p_same`.  Needs labels, every one inside [0, num_classes).  With `augment` (an ``Augment``) the two
        clips of a pair are augmented independently."""
        return PairSampler(self, pairs, num_samples, seed, p_same, shuffle, crop, rank, world, log_capacity, augment)

    def eval_sampler(self, batch_size, num_samples, crop="head", seed=0, rank=0, world=1, top_k=5, sweep_capacity=16):
        """The sweeps of a held-out evaluation (``WaveNet.evaluate``, ``WaveNet.fit(..., validate=...)``): every record once
        per sweep, in order, `batch_size` per step with a ragged last step; the results of the last `sweep_capacity` sweeps
        stay on the device.  Needs labels, every one inside [0, num_classes), and at most 256 classes."""
        return EvalSampler(self, batch_size, num_samples, crop, seed, rank, world, top_k, sweep_capacity)

    def embed_sampler(self, batch_size, num_samples, crop="head", seed=0, bins=512, d_max=None, sweep_capacity=4, rank=0,
                      world=1):
        """The sweeps of a held-out evaluation of an embedding model (``SiameseWaveNet.evaluate``,
        ``SiameseWaveNet.fit(..., validate=...)``): every record once per sweep, in order, then one launch over all pairs
        of records; the results of the last `sweep_capacity` sweeps stay on the device.  `bins` histogram bins over
        [0, `d_max`] (None: twice the model's margin).  Needs labels, every one inside [0, num_classes), at most
        ``MAX_EMBED_RECORDS`` records and world = 1."""
        return EmbedSampler(self, batch_size, num_samples, crop, seed, bins, d_max, sweep_capacity, rank, world)

    def class_index(self):
        """``class_index`` of the labels as device tensors (order, place, start), built and uploaded on first use."""
        if getattr(self, "_class_index", None) is None:
            import torch
            self._class_index = tuple(torch.as_tensor(a).to(self.device)
                                      for a in class_index(self._host_labels(), self.num_classes))
        return self._class_index

    def _host_labels(self) -> np.ndarray:
        if self.labels is None:
            raise ValueError("this dataset holds no labels")
        if getattr(self, "_labels_host", None) is None:
            self._labels_host = self.labels.cpu().numpy()
        return self._labels_host


def _amplitude_range(r, name) -> Tuple[float, float]:
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError("%s %r: a range (lo, hi)" % (name, r))
    with np.errstate(over="ignore"):             # (a value beyond fp32's range is not finite where the kernel reads it)
        finite = np.isfinite(np.float32(lo)) and np.isfinite(np.float32(hi))
    if not (finite and 0.0 <= lo <= hi):
        raise ValueError("%s %r: finite linear amplitudes, 0 <= lo <= hi" % (name, r))
    return lo, hi


class Augment(object):
    """What an augmenting sampler does to every drawn row, immutable: a shift uniform on [-shift, shift] samples with zero
    fill, a gain uniform on ``gain`` and, with probability ``noise_prob``, a window of a clip of the ``DeviceDataset``
    ``noise`` (its labels are unused) added at a volume uniform on ``noise_volume``.  Amplitudes are linear.  The defaults
    change nothing but the sign of a zero (``augment_rows``).

    ``speed=(lo, hi)``, 0.5 <= lo <= hi <= 2: before all that the row is resampled by a factor s of its own, ``y(j) =
    x(j * s)`` -- s > 1 plays faster and higher, by ``12 log2(s)`` semitones, and the content ends at T / s -- through a
    windowed-sinc table of ``taps`` taps (even, 2 .. 64) per phase, cut off for the fastest speed (``resample_table``).
    The row's step is uniform on the fixed-point steps ``[step_lo, step_hi] = round(speed * 2^24)`` (``speed_plan``).

    ``reverb``, a ``DeviceDataset`` whose clips are room impulse responses ``[M, K]``, K at most ``ROOM_MAX_TAPS`` (its
    labels are unused): with probability ``reverb_prob`` the resampled row is convolved with one of them, cut at the row's
    length (``reverb_plan``, ``reverb_rows``), before shift, gain and noise -- the noise is added dry.  ``prepare_rirs``
    brings measured responses into the form a draw wants; ``synthetic_rirs`` makes some up."""
    __slots__ = ("shift", "gain", "noise", "noise_prob", "noise_volume", "noise_threshold", "speed", "taps", "step_lo",
                 "step_hi", "reverb", "reverb_prob", "reverb_threshold")

    def __init__(self, shift=0, gain=(1.0, 1.0), noise=None, noise_prob=0.0, noise_volume=(0.0, 0.0), speed=(1.0, 1.0),
                 taps=16, reverb=None, reverb_prob=0.0):
        if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not 0 <= int(shift) < 1 << 31:
            raise ValueError("shift %r: a number of samples, at least 0" % (shift,))
        if noise is not None and not isinstance(noise, DeviceDataset):
            raise TypeError("noise must be a DeviceDataset of background clips, got %s" % type(noise).__name__)
        set_ = object.__setattr__
        set_(self, "shift", int(shift))
        set_(self, "gain", _amplitude_range(gain, "gain"))
        set_(self, "noise_volume", _amplitude_range(noise_volume, "noise_volume"))
        try:
            set_(self, "noise_threshold", same_threshold(noise_prob))
        except (TypeError, ValueError):
            raise ValueError("noise_prob %r: a probability" % (noise_prob,))
        if noise is None and self.noise_threshold:
            raise ValueError("noise_prob %r without noise: pass the background clips as noise=DeviceDataset(...)"
                             % (noise_prob,))
        set_(self, "noise", noise)
        set_(self, "noise_prob", float(noise_prob))
        try:
            lo, hi = (float(v) for v in speed)
        except (TypeError, ValueError):
            raise ValueError("speed %r: a range (lo, hi)" % (speed,))
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.5 <= lo <= hi <= 2.0):
            raise ValueError("speed %r: finite factors, 0.5 <= lo <= hi <= 2" % (speed,))
        if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not 2 <= int(taps) <= 64 or int(taps) % 2:
            raise ValueError("taps %r: an even number of taps, 2 to 64" % (taps,))
        set_(self, "speed", (lo, hi))
        set_(self, "taps", int(taps))
        set_(self, "step_lo", int(round(lo * SPEED_ONE)))
        set_(self, "step_hi", int(round(hi * SPEED_ONE)))
        if reverb is not None and not isinstance(reverb, DeviceDataset):
            raise TypeError("reverb must be a DeviceDataset of room impulse responses, got %s" % type(reverb).__name__)
        try:
            set_(self, "reverb_threshold", same_threshold(reverb_prob))
        except (TypeError, ValueError):
            raise ValueError("reverb_prob %r: a probability" % (reverb_prob,))
        if reverb is None and self.reverb_threshold:
            raise ValueError("reverb_prob %r without reverb: pass the room impulse responses as reverb=DeviceDataset(...)"
                             % (reverb_prob,))
        set_(self, "reverb", reverb)
        set_(self, "reverb_prob", float(reverb_prob))

    def __setattr__(self, name, value=None):
        raise AttributeError("an Augment is immutable")

    __delattr__ = __setattr__

    def __repr__(self):
        return "Augment(shift=%d, gain=%r, noise=%s, noise_prob=%r, noise_volume=%r%s%s)" % (
            self.shift, self.gain, "None" if self.noise is None else "<%d clips>" % len(self.noise), self.noise_prob,
            self.noise_volume, ", speed=%r, taps=%d" % (self.speed, self.taps) if self.resamples else "",
            ", reverb=<%d responses of %d taps>, reverb_prob=%r" % (len(self.reverb), self.reverb.clip_len, self.reverb_prob)
            if self.reverberates else "")

    @property
    def resamples(self) -> bool:
        """Whether a draw resamples its rows: any speed but exactly (1, 1) (then the draw is the ``_aug`` entry's)."""
        return (self.step_lo, self.step_hi) != (SPEED_ONE, SPEED_ONE)

    @property
    def reverberates(self) -> bool:
        """Whether a draw may reverberate a row: there are responses and the probability is not zero (then the draw is the
        ``_room`` entry's; otherwise it is the entry it was without the two keywords)."""
        return self.reverb is not None and self.reverb_threshold != 0

    @property
    def cutoff(self) -> float:
        """The table's cutoff as a fraction of Nyquist: ``min(1, 1 / hi)``, so the fastest speed folds nothing back."""
        return min(1.0, 1.0 / self.speed[1])

    def table(self) -> np.ndarray:
        """``resample_table(cutoff, taps)``: the one table of this Augment."""
        return resample_table(self.cutoff, self.taps)

    def check(self, dataset, num_samples: int) -> None:
        """What only a sampler knows: the shift stays inside the row, the noise lives beside the clips and covers a row,
        the room responses live there too, are short enough for the kernel and finite (one reduction on the device)."""
        if self.shift >= int(num_samples):
            raise ValueError("augment: shift %d: below num_samples %d" % (self.shift, int(num_samples)))
        if self.noise is not None:
            if str(self.noise.device) != str(dataset.device):
                raise ValueError("augment: the noise is on %s, the clips are on %s" % (self.noise.device, dataset.device))
            if self.noise.clip_len < int(num_samples):
                raise ValueError("augment: noise clips of %d samples are shorter than num_samples %d"
                                 % (self.noise.clip_len, int(num_samples)))
        if self.reverb is not None:
            if str(self.reverb.device) != str(dataset.device):
                raise ValueError("augment: the room responses are on %s, the clips are on %s"
                                 % (self.reverb.device, dataset.device))
            if not 1 <= self.reverb.clip_len <= ROOM_MAX_TAPS:
                raise ValueError("augment: room responses of %d taps: 1 to %d" % (self.reverb.clip_len, ROOM_MAX_TAPS))
            import torch
            if not bool(torch.isfinite(self.reverb.audio).all()):
                raise ValueError("augment: the room responses hold a tap that is not finite")


AugmentPlan = namedtuple("AugmentPlan", "shift gain mix noise_index noise_offset volume")


def _amplitude(h: int, lo: float, hi: float) -> np.float32:
    """lo + u (hi - lo) at u = float32(h >> 40) * 2^-24 (exact): the subtraction, the product and the sum round to fp32."""
    u = np.float32(h >> 40) * np.float32(2.0 ** -24)
    lo, hi = np.float32(lo), np.float32(hi)
    return np.float32(lo + np.float32(u * np.float32(hi - lo)))


def augment_plan(seed: int, step: int, batch_size: int, num_samples: int, augment: "Augment", noise_n: int, noise_len: int,
                 rank: int = 0, world: int = 1, side: int = 0) -> "AugmentPlan":
    """The augmentation of the rows of ``step``: ``(shift [B] int32, gain [B] float32, mix [B] bool, noise_index [B] int32,
    noise_offset [B] int64, volume [B] float32)``.  Row b is ``draw_plan``'s position p = (step * world + rank) * B + b;
    every quantity has a draw of its own, ``_mix64((seed ^ SALT) + _GOLDEN * (2 * p + side + 1))`` with the six AUG salts,
    so ranks, steps, rows and the two sides of a pair never share one.  shift = ``((h >> 32) * (2 S + 1)) >> 32`` minus S;
    gain and volume are ``_amplitude`` of their ranges; mix says the coin ``h >> 32`` lies below ``floor(noise_prob * 2^32)``
    (never without noise clips: `noise_n` 0); the noise record is uniform on [0, noise_n) and its window starts at an
    offset uniform on [0, noise_len - num_samples], both by ``((h >> 32) * range) >> 32``.  `side`: 0 for a ``BatchSampler``
    and the left clip of a pair, 1 for the right clip."""
    batch_size, num_samples, noise_n, noise_len = int(batch_size), int(num_samples), int(noise_n), int(noise_len)
    if not isinstance(augment, Augment):
        raise TypeError("augment must be an Augment, got %s" % type(augment).__name__)
    if not 1 <= batch_size <= MAX_BATCH:
        raise ValueError("batch_size %d: at least 1, at most %d" % (batch_size, MAX_BATCH))
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of %d" % (rank, world))
    if side not in (0, 1):
        raise ValueError("side %r: 0 or 1" % (side,))
    if not augment.shift < num_samples:
        raise ValueError("augment: shift %d: below num_samples %d" % (augment.shift, num_samples))
    if noise_n < 0 or (noise_n > 0 and noise_len < num_samples):
        raise ValueError("augment_plan: %d noise clips of %d samples, num_samples %d" % (noise_n, noise_len, num_samples))
    seed &= _MASK
    S = augment.shift
    plan = AugmentPlan(np.zeros(batch_size, np.int32), np.zeros(batch_size, np.float32), np.zeros(batch_size, bool),
                       np.zeros(batch_size, np.int32), np.zeros(batch_size, np.int64), np.zeros(batch_size, np.float32))
    for b in range(batch_size):
        p = (step * world + rank) * batch_size + b
        h = lambda salt: _mix64((seed ^ salt) + _GOLDEN * (2 * p + side + 1))
        plan.shift[b] = (((h(AUG_SHIFT_SALT) >> 32) * (2 * S + 1)) >> 32) - S
        plan.gain[b] = _amplitude(h(AUG_GAIN_SALT), *augment.gain)
        plan.volume[b] = _amplitude(h(AUG_VOLUME_SALT), *augment.noise_volume)
        if noise_n > 0:
            plan.mix[b] = (h(AUG_COIN_SALT) >> 32) < augment.noise_threshold
            plan.noise_index[b] = ((h(AUG_PICK_SALT) >> 32) * noise_n) >> 32
            plan.noise_offset[b] = ((h(AUG_OFFSET_SALT) >> 32) * (noise_len - num_samples + 1)) >> 32
    return plan


def augment_rows(rows, plan: "AugmentPlan", noise_clips=None) -> np.ndarray:
    """The sample rule on the cropped rows ``[B, T]``, in fp32: ``xs[j] = rows[j - shift]`` inside the row and +0 outside
    (TensorFlow speech_commands' time shift with zero fill, inside the crop window); ``n[j] = noise_clips[noise_index,
    noise_offset + j]`` and v = volume where ``mix``, else n = +0 and v = +0; ``y = fp32(fp32(gain * xs) + fp32(v * n))``,
    then ``y < -1 ? -1 : (y > 1 ? 1 : y)`` (a NaN passes).  The sum is formed with mixing off too, so a zero has one sign
    whatever the plan: -0.0 only where both products are -0.0.  Every destination of a draw holds y."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] != plan.shift.shape[0]:
        raise ValueError("rows must be [%d, T], got %s" % (plan.shift.shape[0], tuple(x.shape)))
    B, T = x.shape
    if plan.mix.any():
        if noise_clips is None:
            raise ValueError("the plan mixes noise into %d rows: pass the noise clips" % int(plan.mix.sum()))
        noise_clips = np.asarray(noise_clips, dtype=np.float32)
    out = np.empty_like(x)
    j = np.arange(T)
    for b in range(B):
        k = j - int(plan.shift[b])
        inside = (k >= 0) & (k < T)
        xs = np.where(inside, x[b, np.clip(k, 0, T - 1)], np.float32(0.0)).astype(np.float32)
        if plan.mix[b]:
            o = int(plan.noise_offset[b])
            n, v = noise_clips[int(plan.noise_index[b]), o:o + T], np.float32(plan.volume[b])
        else:
            n, v = np.zeros(T, np.float32), np.float32(0.0)
        with np.errstate(all="ignore"):
            y = (np.float32(plan.gain[b]) * xs).astype(np.float32) + (v * n).astype(np.float32)
        out[b] = np.where(y < np.float32(-1.0), np.float32(-1.0), np.where(y > np.float32(1.0), np.float32(1.0), y))
    return out


def speed_plan(seed: int, step: int, batch_size: int, augment: "Augment", rank: int = 0, world: int = 1,
               side: int = 0) -> np.ndarray:
    """The fixed-point resampling steps of the rows of ``step``, int64 [B]: row b at ``draw_plan``'s position p draws
    ``h = _mix64((seed ^ AUG_SPEED_SALT) + _GOLDEN * (2 * p + side + 1))`` -- the key of ``augment_plan``'s six draws under
    a seventh salt, so none of them moves -- and its step is ``step_lo + (((h >> 32) * (step_hi - step_lo + 1)) >> 32)``,
    uniform on the integers [step_lo, step_hi].  A step q means speed q / 2^24: no float decides a position."""
    batch_size = int(batch_size)
    if not isinstance(augment, Augment):
        raise TypeError("augment must be an Augment, got %s" % type(augment).__name__)
    if not 1 <= batch_size <= MAX_BATCH:
        raise ValueError("batch_size %d: at least 1, at most %d" % (batch_size, MAX_BATCH))
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of %d" % (rank, world))
    if side not in (0, 1):
        raise ValueError("side %r: 0 or 1" % (side,))
    seed &= _MASK
    lo_q, hi_q = augment.step_lo, augment.step_hi
    out = np.empty(batch_size, np.int64)
    for b in range(batch_size):
        p = (step * world + rank) * batch_size + b
        h = _mix64((seed ^ AUG_SPEED_SALT) + _GOLDEN * (2 * p + side + 1))
        out[b] = lo_q + (((h >> 32) * (hi_q - lo_q + 1)) >> 32)
    return out


_TABLES = {}


def resample_table(cutoff: float, taps: int) -> np.ndarray:
    """The polyphase low-pass of ``resample_rows``, float32 [RESAMPLE_PHASES, taps], read-only.  Tap k of phase f sits at
    distance ``d = k - (taps / 2 - 1) - f / RESAMPLE_PHASES`` samples from the position and weighs ``cutoff * sinc(cutoff *
    d)`` under a Kaiser window of ``RESAMPLE_BETA`` over |d| <= taps / 2, in float64; every phase row is then divided by
    its sum (a constant passes unchanged at any phase) and rounded once to float32.  `cutoff` is a fraction of Nyquist in
    (0, 1]; at 1 phase 0 is written as the exact unit impulse (its sinc has its zeros on the other taps up to rounding)."""
    cutoff, taps = float(cutoff), int(taps)
    if not 0.0 < cutoff <= 1.0:
        raise ValueError("cutoff %r: a fraction of Nyquist in (0, 1]" % (cutoff,))
    if not 2 <= taps <= 64 or taps % 2:
        raise ValueError("taps %r: an even number of taps, 2 to 64" % (taps,))
    if (cutoff, taps) not in _TABLES:
        half = taps // 2
        d = (np.arange(taps, dtype=np.float64) - (half - 1))[None, :] - \
            (np.arange(RESAMPLE_PHASES, dtype=np.float64) / RESAMPLE_PHASES)[:, None]
        w = np.i0(RESAMPLE_BETA * np.sqrt(np.maximum(0.0, 1.0 - (d / half) ** 2))) / np.i0(RESAMPLE_BETA)
        h = cutoff * np.sinc(cutoff * d) * w
        h /= h.sum(axis=1, keepdims=True)
        if cutoff == 1.0:
            h[0] = 0.0
            h[0, half - 1] = 1.0
        t = h.astype(np.float32)
        t.setflags(write=False)
        _TABLES[(cutoff, taps)] = t
    return _TABLES[(cutoff, taps)]


def resample_rows(rows, steps, table) -> np.ndarray:
    """The resampling rule on the cropped rows ``[B, T]``, in fp32 with integer positions.  With P = RESAMPLE_PHASES and
    ``q = j * steps[b]`` (an unsigned 64-bit integer): ``i = q >> 24`` is the source sample at or before the position and
    ``f = (q >> (24 - log2 P)) & (P - 1)`` the phase, selected by floor.  ``r[j]`` is accumulated in tap order k = 0 ..
    taps - 1 from +0.0: ``acc = fp32(acc + fp32(table[f, k] * x[i - (taps / 2 - 1) + k]))``, every operation rounded
    separately, with x = +0.0 outside [0, T) of the row -- samples of the record beyond the crop window are never read.
    The position is anchored at the row's first sample: r[0] filters around x[0], and a row played faster ends at T / s
    with zeros behind (kws_streaming's resample, then pad or crop at the end)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    steps = np.asarray(steps, dtype=np.int64).reshape(-1)
    table = np.asarray(table, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] != steps.shape[0]:
        raise ValueError("rows must be [%d, T], got %s" % (steps.shape[0], tuple(x.shape)))
    if table.ndim != 2 or table.shape[0] != RESAMPLE_PHASES or table.shape[1] % 2 or not 2 <= table.shape[1] <= 64:
        raise ValueError("table must be [%d, taps], got %s" % (RESAMPLE_PHASES, tuple(table.shape)))
    if steps.min() < SPEED_ONE // 2 or steps.max() > 2 * SPEED_ONE:
        raise ValueError("steps outside [2^23, 2^25]")
    B, T = x.shape
    taps = table.shape[1]
    shift = SPEED_BITS - (RESAMPLE_PHASES.bit_length() - 1)
    out = np.empty_like(x)
    j = np.arange(T, dtype=np.uint64)
    for b in range(B):
        q = j * np.uint64(steps[b])
        i = (q >> np.uint64(SPEED_BITS)).astype(np.int64)
        f = ((q >> np.uint64(shift)) & np.uint64(RESAMPLE_PHASES - 1)).astype(np.int64)
        acc = np.zeros(T, np.float32)
        with np.errstate(all="ignore"):
            for k in range(taps):
                at = i - (taps // 2 - 1) + k
                xk = np.where((at >= 0) & (at < T), x[b, np.clip(at, 0, T - 1)], np.float32(0.0)).astype(np.float32)
                acc = (acc + (table[f, k] * xk).astype(np.float32)).astype(np.float32)
        out[b] = acc
    return out


ReverbPlan = namedtuple("ReverbPlan", "apply index")


def reverb_plan(seed: int, step: int, batch_size: int, augment: "Augment", rir_n: int, rank: int = 0, world: int = 1,
                side: int = 0) -> "ReverbPlan":
    """The reverberation of the rows of ``step``: ``(apply [B] bool, index [B] int32)``.  Row b at ``draw_plan``'s position
    p takes two more draws under the key of the other seven, ``h = _mix64((seed ^ SALT) + _GOLDEN * (2 * p + side + 1))``
    with ``AUG_RIR_COIN_SALT`` and ``AUG_RIR_PICK_SALT``, so none of those moves: ``apply = (h_coin >> 32) <
    floor(reverb_prob * 2^32)`` (never without responses: `rir_n` 0) and ``index = ((h_pick >> 32) * rir_n) >> 32``, uniform
    on [0, rir_n)."""
    batch_size, rir_n = int(batch_size), int(rir_n)
    if not isinstance(augment, Augment):
        raise TypeError("augment must be an Augment, got %s" % type(augment).__name__)
    if not 1 <= batch_size <= MAX_BATCH:
        raise ValueError("batch_size %d: at least 1, at most %d" % (batch_size, MAX_BATCH))
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of %d" % (rank, world))
    if side not in (0, 1):
        raise ValueError("side %r: 0 or 1" % (side,))
    if rir_n < 0:
        raise ValueError("reverb_plan: %d room responses" % rir_n)
    seed &= _MASK
    plan = ReverbPlan(np.zeros(batch_size, bool), np.zeros(batch_size, np.int32))
    for b in range(batch_size):
        p = (step * world + rank) * batch_size + b
        h = lambda salt: _mix64((seed ^ salt) + _GOLDEN * (2 * p + side + 1))
        if rir_n > 0:
            plan.apply[b] = (h(AUG_RIR_COIN_SALT) >> 32) < augment.reverb_threshold
            plan.index[b] = ((h(AUG_RIR_PICK_SALT) >> 32) * rir_n) >> 32
    return plan


def reverb_rows(rows, plan: "ReverbPlan", rirs) -> np.ndarray:
    """The reverberation rule on the (cropped, resampled) rows ``[B, T]``, in fp32.  Where ``plan.apply[b]``, with ``h =
    rirs[plan.index[b]]`` of K taps: ``e[j]`` is accumulated in tap order k = 0 .. K - 1 from +0.0, ``acc = fp32(acc +
    fp32(h[k] * r[j - k]))``, every product and every sum rounded separately, with r = +0.0 outside [0, T) -- the record
    before the crop window is never read -- and the tail beyond T is cut.  Elsewhere the row passes untouched, bit for bit.
    In-order sums are the rule because NumPy can state them: a pairwise or fused sum has other bits."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] != plan.apply.shape[0]:
        raise ValueError("rows must be [%d, T], got %s" % (plan.apply.shape[0], tuple(x.shape)))
    out = x.copy()
    if not plan.apply.any():
        return out
    rirs = np.asarray(rirs, dtype=np.float32)
    if rirs.ndim != 2 or not 1 <= rirs.shape[1] <= ROOM_MAX_TAPS:
        raise ValueError("rirs must be [M, K] with 1 <= K <= %d, got %s" % (ROOM_MAX_TAPS, tuple(rirs.shape)))
    B, T = x.shape
    K = rirs.shape[1]
    for b in np.nonzero(plan.apply)[0]:
        h = rirs[int(plan.index[b])]
        padded = np.concatenate([np.zeros(K - 1, np.float32), x[b]])       # padded[K - 1 + i] = r[i]
        acc = np.zeros(T, np.float32)
        with np.errstate(all="ignore"):
            for k in range(K):
                acc = (acc + (h[k] * padded[K - 1 - k:K - 1 - k + T]).astype(np.float32)).astype(np.float32)
        out[b] = acc
    return out


def prepare_rirs(rirs, length: int) -> np.ndarray:
    """Measured room impulse responses ``[M, any]`` (or one, ``[any]``) as a draw wants them, float32 ``[M, length]``,
    computed in float64: what precedes each response's largest |tap| -- the direct path -- is dropped, so reverberation
    does not delay the signal; the rest is cut or zero-padded to `length` and scaled to unit energy, so it does not change
    the level of white input.  A response with a tap that is not finite, or with none that is not zero, is refused."""
    h = np.atleast_2d(np.asarray(rirs, dtype=np.float64))
    length = int(length)
    if h.ndim != 2 or h.shape[1] < 1:
        raise ValueError("rirs must be [M, taps], got %s" % (tuple(np.shape(rirs)),))
    if not 1 <= length <= ROOM_MAX_TAPS:
        raise ValueError("length %d: 1 to %d taps" % (length, ROOM_MAX_TAPS))
    out = np.zeros((h.shape[0], length), np.float64)
    for m in range(h.shape[0]):
        if not np.isfinite(h[m]).all():
            raise ValueError("response %d holds a tap that is not finite" % m)
        if not h[m].any():
            raise ValueError("response %d is all zero" % m)
        d = h[m, int(np.argmax(np.abs(h[m]))):][:length]
        out[m, :d.shape[0]] = d / np.sqrt(np.sum(d * d))
    return out.astype(np.float32)


def synthetic_rirs(n: int, length: int, rt60=(0.2, 0.6), sample_rate: int = 16000, seed: int = 0) -> np.ndarray:
    """`n` made-up room responses, float32 ``[n, length]``: seeded Gaussian noise under ``exp(-6.908 t / rt60)`` -- the
    energy falls by 60 dB in rt60 seconds -- with rt60 uniform on the range and a unit first tap (the direct path), passed
    through ``prepare_rirs``.  For the drivers, the benchmarks and the tests; a real corpus goes through ``prepare_rirs``."""
    n, length = int(n), int(length)
    try:
        lo, hi = (float(v) for v in rt60)
    except (TypeError, ValueError):
        raise ValueError("rt60 %r: a range (lo, hi) of seconds" % (rt60,))
    if n < 1 or not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi) or sample_rate <= 0:
        raise ValueError("synthetic_rirs: n=%d, rt60=%r, sample_rate=%r" % (n, rt60, sample_rate))
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64) / float(sample_rate)
    h = rng.standard_normal((n, length)) * np.exp(-6.908 * t[None, :] / rng.uniform(lo, hi, (n, 1)))
    h[:, 0] = 1.0
    return prepare_rirs(h, length)


def add_augment_flags(parser) -> None:
    """The drivers' augmentation flags (examples/classifier.py, examples/siamese.py); ``augment_from_flags`` reads them."""
    g = parser.add_argument_group("augmentation (--device-data)")
    g.add_argument("--shift", type=int, default=0, metavar="N", help="shift every drawn clip by up to N samples, zero fill")
    g.add_argument("--gain", type=str, default=None, metavar="LO:HI", help="scale every drawn clip by a gain uniform on [LO, HI]")
    g.add_argument("--noise", type=str, default=None, metavar="FILE.npy", help="background clips to mix in: an [M, len] array")
    g.add_argument("--noise-prob", type=float, default=0.0, metavar="P", help="mix noise into a drawn clip with probability P")
    g.add_argument("--noise-volume", type=str, default=None, metavar="LO:HI", help="volume of the noise, uniform on [LO, HI]")
    g.add_argument("--speed", type=str, default=None, metavar="LO:HI",
                   help="resample every drawn clip by a factor uniform on [LO, HI] within [0.5, 2]: tempo and pitch together")
    g.add_argument("--resample-taps", type=int, default=None, metavar="N", help="taps of the resampling filter (even, 2..64; 16)")
    g.add_argument("--rir", type=str, default=None, metavar="FILE.npy",
                   help="room impulse responses to reverberate with: an [M, K] array, K <= %d (dataset.prepare_rirs)" % ROOM_MAX_TAPS)
    g.add_argument("--rir-prob", type=float, default=0.0, metavar="P", help="reverberate a drawn clip with probability P")


def _flag_range(text, name):
    try:
        lo, hi = (float(v) for v in text.split(":"))
    except ValueError:
        raise SystemExit("--%s %r: LO:HI" % (name, text))
    return lo, hi


def augment_from_flags(args, device_data: bool, device="cuda") -> Optional["Augment"]:
    """The ``Augment`` the flags of ``add_augment_flags`` ask for, or None when none of them is set.  They act in the draw
    launch, so without --device-data they are refused here, not ignored.  The noise file is uploaded once."""
    asked = [f for f, on in (("--shift", args.shift != 0), ("--gain", args.gain is not None), ("--noise", args.noise is not None),
                             ("--noise-prob", args.noise_prob != 0.0), ("--noise-volume", args.noise_volume is not None),
                             ("--speed", getattr(args, "speed", None) is not None),
                             ("--resample-taps", getattr(args, "resample_taps", None) is not None),
                             ("--rir", getattr(args, "rir", None) is not None),
                             ("--rir-prob", getattr(args, "rir_prob", 0.0) != 0.0)) if on]
    if not asked:
        return None
    if not device_data:
        raise SystemExit("%s: augmentation happens where the batch is drawn on the device; add --device-data"
                         % ", ".join(asked))
    noise = None
    if args.noise is not None:
        clips = np.load(args.noise)
        if clips.ndim != 2:
            raise SystemExit("--noise %s: an [M, len] array of background clips, got shape %s" % (args.noise, clips.shape))
        noise = DeviceDataset(clips.astype(np.float32), device=device)
    reverb = None
    if getattr(args, "rir", None) is not None:
        rirs = np.load(args.rir)
        if rirs.ndim != 2:
            raise SystemExit("--rir %s: an [M, K] array of room impulse responses, got shape %s" % (args.rir, rirs.shape))
        reverb = DeviceDataset(rirs.astype(np.float32), device=device)
    try:
        return Augment(args.shift, (1.0, 1.0) if args.gain is None else _flag_range(args.gain, "gain"), noise,
                       args.noise_prob, (0.0, 0.0) if args.noise_volume is None else _flag_range(args.noise_volume, "noise-volume"),
                       (1.0, 1.0) if getattr(args, "speed", None) is None else _flag_range(args.speed, "speed"),
                       16 if getattr(args, "resample_taps", None) is None else args.resample_taps, reverb,
                       getattr(args, "rir_prob", 0.0))
    except (TypeError, ValueError) as e:
        raise SystemExit("augmentation flags: %s" % e)


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class BatchSampler(object):
    """The draws of one training run on a ``DeviceDataset``.  Owns the device state ``{seed, step}`` (int64 [2]), the
    loss ring of ``log_capacity`` floats and the ``[batch_size]`` int32 indices of the last draw.  A draw is a function of
    ``(seed, step)`` alone, so a resumed sampler continues its sequence: ``seek(step)`` on a sampler built with the saved
    seed -- what a model's ``load_training_state(logdir, sampler=...)`` does -- draws the batches the stopped run would
    have drawn next."""

    augment = None           # an Augment, or None: the plain draw (class default: objects made without __init__ have none)
    _resample_dev = None     # the Augment's resampling table on the clips' device, uploaded by the first draw that needs it

    def __init__(self, dataset, batch_size, num_samples, seed=0, shuffle=True, crop="head", rank=0, world=1,
                 log_capacity=1024, augment=None):
        batch_size, num_samples, rank, world = int(batch_size), int(num_samples), int(rank), int(world)
        _check_draw(batch_size, len(dataset), dataset.clip_len, num_samples, crop, rank, world)
        if int(log_capacity) < 1:
            raise ValueError("log_capacity %d: at least 1" % int(log_capacity))
        if augment is not None:
            if not isinstance(augment, Augment):
                raise TypeError("augment must be an Augment, got %s" % type(augment).__name__)
            augment.check(dataset, num_samples)
        self.augment = augment
        import torch
        self.dataset, self.batch_size, self.num_samples = dataset, batch_size, num_samples
        self.seed, self.shuffle, self.crop, self.rank, self.world = int(seed) & _MASK, bool(shuffle), crop, rank, world
        self.log_capacity = int(log_capacity)
        dev = dataset.device
        signed = self.seed - (1 << 64) if self.seed >> 63 else self.seed
        self.state = torch.tensor([signed, 0], dtype=torch.int64, device=dev)
        self.log = torch.zeros(self.log_capacity, dtype=torch.float32, device=dev)
        self.indices = torch.zeros(batch_size, dtype=torch.int32, device=dev)
        self.step = 0            # the host's copy of the device counter: steps launched so far

    def plan(self, step: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """``draw_plan`` of `step` (default: the next one) for this sampler."""
        d = self.dataset
        return draw_plan(self.seed, self.step if step is None else int(step), self.batch_size, len(d), d.clip_len,
                         self.num_samples, self.shuffle, self.crop, self.rank, self.world)

    def augment_plan(self, step: Optional[int] = None, side: int = 0) -> "AugmentPlan":
        """``augment_plan`` of `step` (default: the next one) for this sampler's ``augment``."""
        if self.augment is None:
            raise ValueError("this sampler does not augment (it was built with augment=None)")
        nz = self.augment.noise
        return augment_plan(self.seed, self.step if step is None else int(step), self.batch_size, self.num_samples,
                            self.augment, 0 if nz is None else len(nz), 0 if nz is None else nz.clip_len, self.rank,
                            self.world, side)

    def _augment_args(self):
        """The augmentation block of the ``_aug`` entries (srwn.h), behind the plain draw's arguments."""
        a = self.augment
        nz = a.noise
        return (a.shift, a.gain[0], a.gain[1], None if nz is None else nz.audio.data_ptr(), 0 if nz is None else len(nz),
                0 if nz is None else nz.clip_len, a.noise_threshold, a.noise_volume[0], a.noise_volume[1])

    def speed_plan(self, step: Optional[int] = None, side: int = 0) -> np.ndarray:
        """``speed_plan`` of `step` (default: the next one) for this sampler's ``augment``."""
        if self.augment is None:
            raise ValueError("this sampler does not augment (it was built with augment=None)")
        return speed_plan(self.seed, self.step if step is None else int(step), self.batch_size, self.augment, self.rank,
                          self.world, side)

    def _resample_args(self):
        """The resampling block of the ``_warp`` entries (srwn.h), behind the augmentation block."""
        a = self.augment
        if self._resample_dev is None:
            import torch
            self._resample_dev = torch.as_tensor(a.table().copy()).to(self.dataset.device)    # (the cached one is read-only)
        return (self._resample_dev.data_ptr(), a.taps, a.step_lo, a.step_hi)

    def reverb_plan(self, step: Optional[int] = None, side: int = 0) -> "ReverbPlan":
        """``reverb_plan`` of `step` (default: the next one) for this sampler's ``augment``."""
        if self.augment is None:
            raise ValueError("this sampler does not augment (it was built with augment=None)")
        rv = self.augment.reverb
        return reverb_plan(self.seed, self.step if step is None else int(step), self.batch_size, self.augment,
                           0 if rv is None else len(rv), self.rank, self.world, side)

    def _room_args(self):
        """The resampling block and the room block of the ``_room`` entries (srwn.h), behind the augmentation block: a
        null table where the speed is (1, 1) -- through the table, phase 0 would turn -0.0 into +0.0.  Uploads nothing:
        the responses live in their ``DeviceDataset``."""
        a = self.augment
        rv = a.reverb
        warp = self._resample_args() if a.resamples else (None, 0, SPEED_ONE, SPEED_ONE)
        return warp + (rv.audio.data_ptr(), len(rv), rv.clip_len, a.reverb_threshold)

    def seek(self, step: int) -> None:
        """Continues the sequence at `step` (a run resumed from a checkpoint): sets the device counter and the host's."""
        if int(step) < 0:
            raise ValueError("step %d" % int(step))
        self.state[1:].fill_(int(step))
        self.step = int(step)

    # ---- the two launches ------------------------------------------------------------------------------------------
    def draw(self, audio, audio2=None, codes=None, quantization_channels=0, onehot=None, onehot_rows=1, onehot_col0=0):
        """srwn_batch_draw (with an ``Augment``: srwn_batch_draw_aug) on the current stream: the step's rows into `audio` ([B, T] fp32; `audio2` the same once
        more), their mu-law codes into `codes` (int32, B * T), the labels' one-hot rows into columns [onehot_col0,
        onehot_col0 + num_classes) of `onehot` ([B * onehot_rows, ld], fp32 or bf16) and the indices into
        ``self.indices``.  Reads the device step; does not tick it (``log`` does)."""
        import torch
        from . import kernels as K
        d, B, T = self.dataset, self.batch_size, self.num_samples
        pa = K._chk(audio, "audio", torch.float32, (B, T))
        pa2 = K._opt(audio2, "audio2", torch.float32, (B, T))
        pc = None
        if codes is not None:
            pc = K._chk(codes, "codes", torch.int32)
            if codes.numel() != B * T:
                raise ValueError("codes: %d elements, expected %d" % (codes.numel(), B * T))
        po, ld, odt = None, 0, 0
        if onehot is not None:
            if d.labels is None:
                raise ValueError("this dataset holds no labels")
            po = K._chk(onehot, "onehot")
            if onehot.ndim != 2 or onehot.shape[0] != B * int(onehot_rows) or \
                    int(onehot_col0) < 0 or int(onehot_col0) + d.num_classes > onehot.shape[1]:
                raise ValueError("onehot: shape %s, expected [%d, >= %d]"
                                 % (tuple(onehot.shape), B * int(onehot_rows), int(onehot_col0) + d.num_classes))
            ld, odt = int(onehot.shape[1]), K.abi_dtype(onehot.dtype)
        args = (d.audio.data_ptr(), None if d.labels is None else d.labels.data_ptr(), len(d),
                d.clip_len, self.state.data_ptr(), B, T, int(self.shuffle), CROPS[self.crop], self.rank, self.world, pa, pa2,
                pc, int(quantization_channels), po, ld, int(onehot_rows), int(onehot_col0), d.num_classes, odt,
                self.indices.data_ptr())
        if self.augment is None:
            K.call("srwn_batch_draw", *args, K._stream())
        elif self.augment.reverberates:      # ... and, where the row's coin says so, through dataset.reverb_rows
            K.call("srwn_batch_draw_room", *args, *self._augment_args(), *self._room_args(), K._stream())
        elif not self.augment.resamples:     # the same rows through dataset.augment_rows, audio, audio2 and codes alike
            K.call("srwn_batch_draw_aug", *args, *self._augment_args(), K._stream())
        else:                                # ... through dataset.resample_rows first
            K.call("srwn_batch_draw_warp", *args, *self._augment_args(), *self._resample_args(), K._stream())

    def log_step(self, loss):
        """srwn_step_log on the current stream: ``log[step % log_capacity] = loss``, then the device step ticks."""
        import torch
        from . import kernels as K
        K.call("srwn_step_log", K._chk(loss, "loss", torch.float32, (1,)), self.log.data_ptr(), self.log_capacity,
               self.state.data_ptr(), K._stream())

    # ---- what ``fit`` asks of a sampler: its log launch for an engine, and the logged steps as arrays --------------------
    def log_engine(self, eng):
        self.log_step(eng.loss)

    def results(self, step0: int, count: int):
        return (self.losses(step0, count),)

    def losses(self, step0: int, count: int) -> np.ndarray:
        """The losses of steps [step0, step0 + count) from the ring (count <= log_capacity): the host waits here."""
        if not 0 <= count <= self.log_capacity:
            raise ValueError("the ring holds %d losses, asked for %d" % (self.log_capacity, count))
        ring = self.log.cpu().numpy()
        return ring[(step0 + np.arange(count)) % self.log_capacity].astype(np.float32)


class DistillSampler(BatchSampler):
    """The draws of a student's distillation run.  Beside a ``BatchSampler``'s state it owns the rings of the power loss
    and the entropy; ``temperature`` scales the noise.  ``draw`` is ``srwn_distill_draw`` (the clips into up to three
    buffers, the noise, the one-hot rows into every conditioning input), ``scatter`` is ``srwn_cond_scatter`` (the
    teacher's encoding into the same inputs), ``log_engine`` is ``srwn_distill_log``."""

    def __init__(self, dataset, batch_size, num_samples, seed=0, shuffle=True, crop="head", temperature=1.0, rank=0,
                 world=1, log_capacity=1024):
        if not np.isfinite(float(temperature)) or float(temperature) < 0.0:
            raise ValueError("temperature %r: finite and not negative" % (temperature,))
        BatchSampler.__init__(self, dataset, batch_size, num_samples, seed, shuffle, crop, rank, world, log_capacity)
        import torch
        self.temperature = float(temperature)
        self.power_log = torch.zeros_like(self.log)
        self.entropy_log = torch.zeros_like(self.log)
        self._tables = None      # (the tensors, their addresses on the device)

    def noise_plan(self, step: Optional[int] = None) -> np.ndarray:
        """``noise_plan`` of `step` (default: the next one) for this sampler."""
        return noise_plan(self.seed, self.step if step is None else int(step), self.batch_size, self.num_samples,
                          self.rank, self.world)

    def noise_rows(self, step: Optional[int] = None) -> np.ndarray:
        return noise_rows(self.seed, self.step if step is None else int(step), self.batch_size, self.rank, self.world)

    def _table_addresses(self, tables):
        import torch
        tables = list(tables)
        if self._tables is None or len(self._tables[0]) != len(tables) or \
                any(a is not b for a, b in zip(self._tables[0], tables)):
            t0 = tables[0]
            for t in tables:
                if t.ndim != 2 or t.shape != t0.shape or t.dtype != t0.dtype or not t.is_contiguous():
                    raise NotImplementedError("the conditioning inputs of one step must share shape and dtype: %s %s, %s %s"
                                              % (tuple(t0.shape), t0.dtype, tuple(t.shape), t.dtype))
            if len(tables) > 64:
                raise ValueError("%d conditioning inputs: at most 64" % len(tables))
            addr = torch.tensor([t.data_ptr() for t in tables], dtype=torch.int64, device=self.dataset.device)
            self._tables = (tables, addr)
        return self._tables[1]

    def draw(self, audio, audio2=None, audio3=None, noise=None, tables=None, rows=1, col0=0):
        """srwn_distill_draw on the current stream: the step's rows into `audio` (and `audio2`, `audio3`: [B, T] fp32), its
        noise times ``temperature`` into `noise` and, with `tables` (matrices [B * rows, ld] of one dtype), the labels'
        one-hot rows into columns [col0, col0 + num_classes) of each.  Reads the device step; does not tick it."""
        import torch
        from . import kernels as K
        d, B, T = self.dataset, self.batch_size, self.num_samples
        pa = K._chk(audio, "audio", torch.float32, (B, T))
        pa2 = K._opt(audio2, "audio2", torch.float32, (B, T))
        pa3 = K._opt(audio3, "audio3", torch.float32, (B, T))
        pn = K._opt(noise, "noise", torch.float32, (B, T))
        pt, nt, ld, dt = None, 0, 0, 0
        if tables:
            if d.labels is None:
                raise ValueError("this dataset holds no labels")
            pt, nt = self._table_addresses(tables).data_ptr(), len(tables)
            t0 = tables[0]
            if t0.shape[0] != B * int(rows) or int(col0) < 0 or int(col0) + d.num_classes > t0.shape[1]:
                raise ValueError("tables: shape %s, expected [%d, >= %d]"
                                 % (tuple(t0.shape), B * int(rows), int(col0) + d.num_classes))
            ld, dt = int(t0.shape[1]), K.abi_dtype(t0.dtype)
        K.call("srwn_distill_draw", d.audio.data_ptr(), None if d.labels is None else d.labels.data_ptr(), len(d),
               d.clip_len, self.state.data_ptr(), B, T, int(self.shuffle), CROPS[self.crop], self.rank, self.world, pa, pa2,
               pa3, pn, self.temperature, pt, nt, ld, int(rows), int(col0), d.num_classes, dt, self.indices.data_ptr(),
               K._stream())

    def scatter(self, enc, tables):
        """srwn_cond_scatter on the current stream: `enc` [rows, latent] fp32 into columns [0, latent) of every table, in
        the tables' dtype -- the bits of ``table[:, :latent].copy_(enc)``."""
        import torch
        from . import kernels as K
        pe = K._chk(enc, "enc", torch.float32)
        t0 = tables[0]
        addr = self._table_addresses(tables)
        if enc.ndim != 2 or enc.shape[0] != t0.shape[0] or enc.shape[1] > t0.shape[1]:
            raise ValueError("enc: shape %s against tables %s" % (tuple(enc.shape), tuple(t0.shape)))
        K.call("srwn_cond_scatter", pe, int(enc.shape[0]), int(enc.shape[1]), addr.data_ptr(), len(tables),
               int(t0.shape[1]), K.abi_dtype(t0.dtype), K._stream())

    def log_engine(self, eng):
        """srwn_distill_log on the current stream, for a ``student.StudentEngine``: loss, power loss and entropy of the step
        into the three rings (``StudentEngine.losses()``'s arithmetic on the device), then the device step ticks."""
        from . import kernels as K
        K.call("srwn_distill_log", eng.ce.data_ptr(), eng.power.data_ptr(), eng.logs.data_ptr(), float(eng.alpha),
               float(eng.beta), int(eng.N), float(eng.loss_div), self.log.data_ptr(), self.power_log.data_ptr(),
               self.entropy_log.data_ptr(), self.log_capacity, self.state.data_ptr(), K._stream())

    def _ring(self, ring, step0, count):
        if not 0 <= count <= self.log_capacity:
            raise ValueError("the ring holds %d steps, asked for %d" % (self.log_capacity, count))
        return ring.cpu().numpy()[(step0 + np.arange(count)) % self.log_capacity].astype(np.float32)

    def power_losses(self, step0: int, count: int) -> np.ndarray:
        return self._ring(self.power_log, step0, count)

    def entropies(self, step0: int, count: int) -> np.ndarray:
        return self._ring(self.entropy_log, step0, count)

    def results(self, step0: int, count: int):
        return self.losses(step0, count), self.power_losses(step0, count)


class PairSampler(BatchSampler):
    """The draws of a twin-tower run on a labelled ``DeviceDataset``: ``pairs`` pairs per step, "same class" with
    probability ``p_same`` (``pair_plan``).  ``batch_size`` is the number of pairs.  Beside the loss ring it owns the
    ``[log_capacity, pairs]`` distance ring and the left indices (``indices``), right indices and y of the last draw."""

    def __init__(self, dataset, pairs, num_samples, seed=0, p_same=0.5, shuffle=True, crop="head", rank=0, world=1,
                 log_capacity=1024, augment=None):
        if dataset.labels is None:
            raise ValueError("pair_sampler: the dataset holds no labels; pairs are drawn by class")
        self.same_threshold = same_threshold(p_same)
        if int(pairs) > 32767:
            raise ValueError("pairs %d: at most 32767" % int(pairs))
        _check_draw(int(pairs), len(dataset), dataset.clip_len, int(num_samples), crop, int(rank), int(world))
        if int(log_capacity) < 1:
            raise ValueError("log_capacity %d: at least 1" % int(log_capacity))
        if augment is not None:
            if not isinstance(augment, Augment):
                raise TypeError("augment must be an Augment, got %s" % type(augment).__name__)
            augment.check(dataset, num_samples)
        self._index = dataset.class_index()          # (refuses labels outside the classes)
        BatchSampler.__init__(self, dataset, pairs, num_samples, seed, shuffle, crop, rank, world, log_capacity, augment)
        import torch
        dev = dataset.device
        self.pairs, self.p_same = int(pairs), float(p_same)
        self.right = torch.zeros(self.pairs, dtype=torch.int32, device=dev)
        self.y = torch.zeros(self.pairs, dtype=torch.float32, device=dev)
        self.dist_log = torch.zeros((self.log_capacity, self.pairs), dtype=torch.float32, device=dev)

    def pair_plan(self, step: Optional[int] = None):
        """``pair_plan`` of `step` (default: the next one) for this sampler."""
        d = self.dataset
        return pair_plan(self.seed, self.step if step is None else int(step), self.pairs, d._host_labels(), d.num_classes,
                         d.clip_len, self.num_samples, self.p_same, self.shuffle, self.crop, self.rank, self.world)

    def augment_plan(self, step: Optional[int] = None):
        """``(left, right)``: ``augment_plan`` of `step` (default: the next one) for the pairs' left clips (side 0) and
        right clips (side 1)."""
        return BatchSampler.augment_plan(self, step, 0), BatchSampler.augment_plan(self, step, 1)

    def speed_plan(self, step: Optional[int] = None, side: Optional[int] = None):
        """``speed_plan`` of `step` (default: the next one): ``(left, right)``, or one `side` of the pairs."""
        if side is None:
            return BatchSampler.speed_plan(self, step, 0), BatchSampler.speed_plan(self, step, 1)
        return BatchSampler.speed_plan(self, step, side)

    def reverb_plan(self, step: Optional[int] = None, side: Optional[int] = None):
        """``reverb_plan`` of `step` (default: the next one): ``(left, right)``, or one `side` of the pairs."""
        if side is None:
            return BatchSampler.reverb_plan(self, step, 0), BatchSampler.reverb_plan(self, step, 1)
        return BatchSampler.reverb_plan(self, step, side)

    def draw(self, audio, labels):
        """srwn_pair_draw (with an ``Augment``: srwn_pair_draw_aug) on the current stream: the left clips into rows [0, P) and the right ones into rows [P, 2P) of
        `audio` ([2P, T] fp32), y into `labels` ([P] fp32); the draw's indices and y into ``indices``, ``right``, ``y``."""
        import torch
        from . import kernels as K
        d, P, T = self.dataset, self.pairs, self.num_samples
        order, place, start = self._index
        args = (d.audio.data_ptr(), d.labels.data_ptr(), order.data_ptr(), place.data_ptr(),
                start.data_ptr(), d.num_classes, len(d), d.clip_len, self.state.data_ptr(), P, T, self.same_threshold,
                int(self.shuffle), CROPS[self.crop], self.rank, self.world, K._chk(audio, "audio", torch.float32, (2 * P, T)),
                K._chk(labels, "labels", torch.float32, (P,)), self.indices.data_ptr(), self.right.data_ptr(),
                self.y.data_ptr())
        if self.augment is None:
            K.call("srwn_pair_draw", *args, K._stream())
        elif self.augment.reverberates:
            K.call("srwn_pair_draw_room", *args, *self._augment_args(), *self._room_args(), K._stream())
        elif not self.augment.resamples:
            K.call("srwn_pair_draw_aug", *args, *self._augment_args(), K._stream())
        else:
            K.call("srwn_pair_draw_warp", *args, *self._augment_args(), *self._resample_args(), K._stream())

    def log_pairs(self, loss, dist):
        """srwn_pair_log on the current stream: the loss and the P distances into their rings, then the step ticks."""
        import torch
        from . import kernels as K
        K.call("srwn_pair_log", K._chk(loss, "loss", torch.float32, (1,)), K._chk(dist, "dist", torch.float32, (self.pairs,)),
               self.pairs, self.log.data_ptr(), self.dist_log.data_ptr(), self.log_capacity, self.state.data_ptr(),
               K._stream())

    def log_engine(self, eng):
        self.log_pairs(eng.loss, eng.dist)

    def distances(self, step0: int, count: int) -> np.ndarray:
        """The distances [count, P] of steps [step0, step0 + count) from the ring (count <= log_capacity)."""
        if not 0 <= count <= self.log_capacity:
            raise ValueError("the ring holds %d steps, asked for %d" % (self.log_capacity, count))
        return self.dist_log.cpu().numpy()[(step0 + np.arange(count)) % self.log_capacity].astype(np.float32)

    def results(self, step0: int, count: int):
        return self.losses(step0, count), self.distances(step0, count)


MAX_EVAL_CLASSES = 256     # srwn_eval_classes: a wave per row, four classes per lane


class EvalResult(object):
    """One sweep of a labelled set through a classifier, as NumPy arrays on the host.

    ``pred``, ``rank`` (int32 [N]) and ``nll`` (float32 [N]) per record: the predicted class, the number of classes that
    come before the label's class (0 = correct; top-k accuracy is ``mean(rank < k)``) and -log p(label).  ``confusion``
    int32 [C, C] counts (label, prediction) and ``seen`` the records counted.  ``owned`` bool [N] marks the records this
    rank swept -- all of them with world = 1; elsewhere ``pred`` and ``rank`` are -1 and ``nll`` is NaN.  ``accuracy``,
    ``top_k_accuracy`` (at ``top_k``) and ``mean_nll`` (a float64 sum on the host) are over the owned records;
    ``per_class`` int64 [C, 2] holds (correct, total) per class, the counts train.py:94-113 prints.  ``step`` is the
    training step the sweep was taken at, or None."""

    def __init__(self, pred, rank, nll, confusion, seen, owned, top_k, step=None):
        self.pred, self.rank, self.nll, self.confusion = pred, rank, nll, confusion
        self.seen, self.owned, self.top_k, self.step = int(seen), owned, int(top_k), step
        n = max(self.seen, 1)
        self.accuracy = float(np.trace(confusion)) / n
        self.top_k_accuracy = float(np.count_nonzero(rank[owned] < self.top_k)) / n
        self.mean_nll = float(nll[owned].astype(np.float64).sum()) / n
        self.per_class = np.stack([np.diag(confusion), confusion.sum(axis=1)], axis=1).astype(np.int64)

    def __repr__(self):
        return "EvalResult(step=%r, seen=%d, accuracy=%.4f, top_%d_accuracy=%.4f, mean_nll=%.4f)" % (
            self.step, self.seen, self.accuracy, self.top_k, self.top_k_accuracy, self.mean_nll)


class EvalSampler(BatchSampler):
    """The sweeps of a held-out evaluation on a labelled ``DeviceDataset`` (``sweep_plan``).  A ``BatchSampler`` without
    shuffling that owns the device state ``{seed, step, sweep}`` (int64 [3]) and ``sweep_capacity`` result slots, each
    ``pred [N]`` int32, ``rank [N]`` int32, ``nll [N]`` float32, ``confusion [C, C]`` int32 and ``seen`` int32: sweep k
    lands in slot k % sweep_capacity.  Its draw is ``srwn_batch_draw``; the launch behind the forward pass,
    ``srwn_eval_classes`` (``classify``), writes the slot and ticks the state."""

    def __init__(self, dataset, batch_size, num_samples, crop="head", seed=0, rank=0, world=1, top_k=5, sweep_capacity=16):
        if dataset.labels is None:
            raise ValueError("eval_sampler: the dataset holds no labels; an evaluation counts predictions against them")
        C_ = int(dataset.num_classes)
        if C_ > MAX_EVAL_CLASSES:
            raise ValueError("eval_sampler: num_classes %d: at most %d" % (C_, MAX_EVAL_CLASSES))
        if int(top_k) < 1:
            raise ValueError("top_k %d: at least 1" % int(top_k))
        if int(sweep_capacity) < 1:
            raise ValueError("sweep_capacity %d: at least 1" % int(sweep_capacity))
        _check_draw(int(batch_size), len(dataset), dataset.clip_len, int(num_samples), crop, int(rank), int(world))
        class_index(dataset._host_labels(), C_)              # (refuses labels outside the classes)
        BatchSampler.__init__(self, dataset, batch_size, num_samples, seed, False, crop, rank, world, 1)
        import torch
        dev, n = dataset.device, len(dataset)
        self.top_k, self.sweep_capacity = int(top_k), int(sweep_capacity)
        self.sweep_steps = sweep_steps(n, self.batch_size, self.world)
        self.state = torch.tensor([int(self.state[0]), 0, 0], dtype=torch.int64, device=dev)
        self.pred = torch.zeros((self.sweep_capacity, n), dtype=torch.int32, device=dev)
        self.rank_of_label = torch.zeros((self.sweep_capacity, n), dtype=torch.int32, device=dev)
        self.nll = torch.zeros((self.sweep_capacity, n), dtype=torch.float32, device=dev)
        self.confusion = torch.zeros((self.sweep_capacity, C_, C_), dtype=torch.int32, device=dev)
        self.seen = torch.zeros(self.sweep_capacity, dtype=torch.int32, device=dev)
        self.sweep = 0           # the host's copy of the device's sweep counter: sweeps launched so far

    def plan(self, step: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """``sweep_plan`` of `step` (default: the next one) for this sampler."""
        return sweep_plan(self.step if step is None else int(step), self.batch_size, len(self.dataset), self.rank,
                          self.world)

    def owned(self) -> np.ndarray:
        """bool [N]: the records this rank's sweep visits."""
        own = np.zeros(len(self.dataset), bool)
        for s in range(self.sweep_steps):
            idx, valid = self.plan(s)
            own[idx[valid]] = True
        return own

    def seek(self, step: int) -> None:
        """Continues the current sweep at `step` (0: starts it over): sets the device's step and the host's."""
        if not 0 <= int(step) < self.sweep_steps:
            raise ValueError("step %d of a sweep of %d" % (int(step), self.sweep_steps))
        self.state[1:2].fill_(int(step))
        self.step = int(step)

    def log_step(self, loss):
        raise TypeError("an EvalSampler logs no loss: its last launch is srwn_eval_classes (pass it to evaluate(), or to "
                        "fit(..., validate=(sampler, every)))")

    def classify(self, probs):
        """srwn_eval_classes on the current stream: the step's valid rows of `probs` ([B, C] fp32) into the slot of the
        device's sweep, then the device state ticks."""
        import torch
        from . import kernels as K
        d, B = self.dataset, self.batch_size
        K.call("srwn_eval_classes", K._chk(probs, "probs", torch.float32, (B, d.num_classes)), self.indices.data_ptr(),
               d.labels.data_ptr(), self.state.data_ptr(), len(d), B, d.num_classes, self.rank, self.world,
               self.sweep_capacity, self.pred.data_ptr(), self.rank_of_label.data_ptr(), self.nll.data_ptr(),
               self.confusion.data_ptr(), self.seen.data_ptr(), K._stream())

    def stepped(self) -> None:
        """The host's copy of the tick of one ``classify`` launch (or one replay of a graph that holds it)."""
        self.step += 1
        if self.step >= self.sweep_steps:
            self.step = 0
            self.sweep += 1

    def result(self, sweep: int, step=None) -> "EvalResult":
        """Sweep number `sweep` (one of the last ``sweep_capacity`` completed) from its slot: the host waits here."""
        sweep = int(sweep)
        if not max(0, self.sweep - self.sweep_capacity) <= sweep < self.sweep:
            raise ValueError("sweep %d: the slots hold sweeps [%d, %d)"
                             % (sweep, max(0, self.sweep - self.sweep_capacity), self.sweep))
        k = sweep % self.sweep_capacity
        own = self.owned()
        pred = np.where(own, self.pred[k].cpu().numpy(), np.int32(-1)).astype(np.int32)
        rank = np.where(own, self.rank_of_label[k].cpu().numpy(), np.int32(-1)).astype(np.int32)
        nll = np.where(own, self.nll[k].cpu().numpy(), np.float32(np.nan)).astype(np.float32)
        return EvalResult(pred, rank, nll, self.confusion[k].cpu().numpy(), int(self.seen[k].item()), own, self.top_k, step)


MAX_EMBED_RECORDS = 4096   # srwn_pair_sweep: a workgroup per record keeps the record's row of distances in LDS
MAX_EMBED_BINS = 4096      # ... and two histograms of `bins` counters
MAX_EMBED_DIM = 1024       # ... and the record's own embedding


class PairEvalResult(object):
    """One sweep of a labelled set through an embedding model and over all its pairs, as NumPy arrays on the host.

    ``emb`` float32 [N, D]; per record i over the other records j in the order (distance, index): ``nearest`` and
    ``nearest_dist`` (the first j), ``same_nearest`` and ``same_dist`` (the first j of i's label; -1 and +inf without one)
    and ``rank_same`` (the records of another label in front of ``same_nearest``; -1 without one) -- ``rank_same == 0`` is a
    correct 1-NN classification.  ``hist_same`` / ``hist_diff`` int64 [bins] count the pairs i < j of one label / of two
    labels by ``bin = min(bins - 1, int(d * fp32(bins / d_max)))``.  ``labels`` int32 [N], ``seen`` the records collected,
    ``step`` the training step the sweep was taken at or None, ``distances`` the whole [N, N] matrix or None.

    Every metric is derived from the integers in float64.  Thresholds lie on the bin edges ``edge(k) = (k + 1) * d_max /
    bins`` for k = -1 .. bins - 1: at edge k a pair is accepted as "same" iff its bin <= k, so edge -1 accepts nothing and
    edge bins - 1 everything (the last bin also holds the pairs beyond d_max).  A rate over an empty set of pairs is NaN,
    and so are ``eer``, ``eer_threshold`` and ``auc`` then."""

    def __init__(self, emb, nearest, nearest_dist, same_nearest, same_dist, rank_same, hist_same, hist_diff, seen, labels,
                 bins, d_max, step=None, distances=None):
        self.emb, self.nearest, self.nearest_dist = emb, nearest, nearest_dist
        self.same_nearest, self.same_dist, self.rank_same = same_nearest, same_dist, rank_same
        self.hist_same, self.hist_diff = np.asarray(hist_same, np.int64), np.asarray(hist_diff, np.int64)
        self.seen, self.labels, self.bins, self.d_max = int(seen), labels, int(bins), float(d_max)
        self.step, self.distances = step, distances
        self.nn_accuracy = self.recall_at(1)
        far, frr = self.rates()
        if np.isnan(far).any() or np.isnan(frr).any():
            self.eer = self.eer_threshold = self.auc = float("nan")
        else:
            k = int(np.argmin(np.abs(far - frr)))            # (the first minimum: the lowest edge)
            self.eer = float((far[k] + frr[k]) / 2.0)
            self.eer_threshold = self.edge(k - 1)
            tpr = 1.0 - frr
            self.auc = float(np.sum((far[1:] - far[:-1]) * (tpr[1:] + tpr[:-1]) / 2.0))

    def edge(self, k: int) -> float:
        """The threshold of bin edge k in [-1, bins - 1]."""
        return (int(k) + 1) * self.d_max / self.bins

    def rates(self):
        """``(FAR, FRR)``, float64 [bins + 1]: entry k + 1 is at edge k, from edge -1 (accept nothing: 0, 1) to edge
        bins - 1 (accept everything: 1, 0)."""
        same, diff = self.hist_same.astype(np.float64), self.hist_diff.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            far = np.concatenate([[0.0], np.cumsum(diff)]) / diff.sum()
            frr = (same.sum() - np.concatenate([[0.0], np.cumsum(same)])) / same.sum()
        return far, frr

    def far_frr(self, threshold: float):
        """``(FAR, FRR)`` at a threshold on a bin edge."""
        x = float(threshold) * self.bins / self.d_max
        k = int(round(x)) - 1
        if not -1 <= k <= self.bins - 1 or abs(x - (k + 1)) > 1e-9 * max(1.0, abs(x)):
            raise ValueError("threshold %r: thresholds lie on the bin edges (k + 1) * %r / %d, k in [-1, %d]"
                             % (threshold, self.d_max, self.bins, self.bins - 1))
        far, frr = self.rates()
        return float(far[k + 1]), float(frr[k + 1])

    def recall_at(self, k: int) -> float:
        """``mean(0 <= rank_same < k)`` over all records: a record without a partner of its label counts as a miss."""
        r = self.rank_same
        return float(np.count_nonzero((r >= 0) & (r < int(k)))) / max(int(r.shape[0]), 1)

    def __repr__(self):
        return "PairEvalResult(step=%r, seen=%d, nn_accuracy=%.4f, eer=%.4f at %.4f, auc=%.4f)" % (
            self.step, self.seen, self.nn_accuracy, self.eer, self.eer_threshold, self.auc)


class EmbedSampler(BatchSampler):
    """The sweeps of a held-out evaluation of an embedding model on a labelled ``DeviceDataset`` (``sweep_plan``).  A
    ``BatchSampler`` without shuffling that owns the device state ``{seed, step, sweep}`` (int64 [3]) and ``sweep_capacity``
    result slots, each ``emb [N, D]`` fp32, ``nearest``, ``same_nearest``, ``rank_same`` int32 [N], ``nearest_dist``,
    ``same_dist`` fp32 [N], ``hist_same``, ``hist_diff`` int64 [bins] and ``seen`` int32: sweep k lands in slot
    k % sweep_capacity.  Its draw is ``srwn_batch_draw``; the launch behind the forward pass, ``srwn_embed_collect``
    (``collect``), fills the slot's embeddings and ticks the state; ``srwn_pair_sweep`` (``pair_sweep``) behind a sweep's last
    step fills the rest from all pairs.  D and, with ``d_max=None``, the histograms' range (twice the margin) come from the
    model that first runs the sampler (``bind``).  At most ``MAX_EMBED_RECORDS`` records; world = 1 only."""

    def __init__(self, dataset, batch_size, num_samples, crop="head", seed=0, bins=512, d_max=None, sweep_capacity=4, rank=0,
                 world=1):
        if dataset.labels is None:
            raise ValueError("embed_sampler: the dataset holds no labels; the pairs are counted by them")
        if int(world) > 1:
            raise ValueError("embed_sampler: world %d: the all-pairs pass needs every rank's embeddings, and a rank collects "
                             "only its own share of the records (an all-gather of embeddings is not built): world = 1"
                             % int(world))
        if not 1 <= int(bins) <= MAX_EMBED_BINS:
            raise ValueError("bins %d: at least 1, at most %d" % (int(bins), MAX_EMBED_BINS))
        if d_max is not None and not (np.isfinite(float(d_max)) and float(d_max) > 0.0):
            raise ValueError("d_max %r: finite and above 0" % (d_max,))
        if int(sweep_capacity) < 1:
            raise ValueError("sweep_capacity %d: at least 1" % int(sweep_capacity))
        if len(dataset) > MAX_EMBED_RECORDS:
            raise ValueError("embed_sampler: %d records: at most %d (a record's row of distances stays in one workgroup's "
                             "LDS)" % (len(dataset), MAX_EMBED_RECORDS))
        _check_draw(int(batch_size), len(dataset), dataset.clip_len, int(num_samples), crop, int(rank), int(world))
        class_index(dataset._host_labels(), int(dataset.num_classes))      # (refuses labels outside the classes)
        BatchSampler.__init__(self, dataset, batch_size, num_samples, seed, False, crop, rank, world, 1)
        import torch
        dev, n = dataset.device, len(dataset)
        self.bins, self.d_max, self.sweep_capacity = int(bins), None if d_max is None else float(d_max), int(sweep_capacity)
        self.sweep_steps = sweep_steps(n, self.batch_size, self.world)
        self.state = torch.tensor([int(self.state[0]), 0, 0], dtype=torch.int64, device=dev)
        cap = self.sweep_capacity
        self.dim = None          # D, once a model has bound the sampler
        self.emb = None
        self.nearest = torch.zeros((cap, n), dtype=torch.int32, device=dev)
        self.same_nearest = torch.zeros((cap, n), dtype=torch.int32, device=dev)
        self.rank_same = torch.zeros((cap, n), dtype=torch.int32, device=dev)
        self.nearest_dist = torch.zeros((cap, n), dtype=torch.float32, device=dev)
        self.same_dist = torch.zeros((cap, n), dtype=torch.float32, device=dev)
        self.hist_same = torch.zeros((cap, self.bins), dtype=torch.int64, device=dev)
        self.hist_diff = torch.zeros((cap, self.bins), dtype=torch.int64, device=dev)
        self.seen = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.dist = None         # [N, N], allocated by the first sweep that asks for the matrix
        self.sweep = 0           # the host's copy of the device's sweep counter: sweeps launched so far

    def bind(self, dim: int, d_max_default: float) -> None:
        """What the model supplies when it first runs the sampler: the embedding's dimensions (the slots' ``emb`` are
        allocated here) and, where the sampler was built with ``d_max=None``, the histograms' range."""
        dim = int(dim)
        if not 1 <= dim <= MAX_EMBED_DIM:
            raise ValueError("embed_sampler: %d embedding dimensions: at least 1, at most %d" % (dim, MAX_EMBED_DIM))
        if self.dim is not None and self.dim != dim:
            raise ValueError("embed_sampler: bound to %d embedding dimensions, the model has %d" % (self.dim, dim))
        if self.d_max is None:
            if not (np.isfinite(float(d_max_default)) and float(d_max_default) > 0.0):
                raise ValueError("d_max %r: finite and above 0" % (d_max_default,))
            self.d_max = float(d_max_default)
        if self.dim is None:
            import torch
            self.dim = dim
            self.emb = torch.zeros((self.sweep_capacity, len(self.dataset), dim), dtype=torch.float32,
                                   device=self.dataset.device)

    @property
    def scale(self) -> np.float32:
        """fp32(bins / d_max): what ``srwn_pair_sweep`` multiplies a distance by."""
        if self.d_max is None:
            raise ValueError("embed_sampler: d_max is not set yet (the model supplies 2 * margin when it first runs the sampler)")
        return np.float32(self.bins / self.d_max)

    def plan(self, step: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """``sweep_plan`` of `step` (default: the next one) for this sampler."""
        return sweep_plan(self.step if step is None else int(step), self.batch_size, len(self.dataset), self.rank,
                          self.world)

    def seek(self, step: int) -> None:
        """Continues the current sweep at `step` (0: starts it over): sets the device's step and the host's."""
        if not 0 <= int(step) < self.sweep_steps:
            raise ValueError("step %d of a sweep of %d" % (int(step), self.sweep_steps))
        self.state[1:2].fill_(int(step))
        self.step = int(step)

    def log_step(self, loss):
        raise TypeError("an EmbedSampler logs no loss: its last launch is srwn_embed_collect (pass it to "
                        "SiameseWaveNet.evaluate(), or to fit(..., validate=(sampler, every)))")

    def collect(self, emb):
        """srwn_embed_collect on the current stream: the step's valid rows of `emb` ([B, D] fp32) into the slot of the
        device's sweep, then the device state ticks."""
        import torch
        from . import kernels as K
        d, B = self.dataset, self.batch_size
        if self.emb is None:
            raise ValueError("embed_sampler: not bound to a model yet (bind)")
        K.call("srwn_embed_collect", K._chk(emb, "emb", torch.float32, (B, self.dim)), self.indices.data_ptr(),
               self.state.data_ptr(), len(d), B, self.dim, self.rank, self.world, self.sweep_capacity, self.emb.data_ptr(),
               self.seen.data_ptr(), K._stream())

    def stepped(self) -> None:
        """The host's copy of the tick of one ``collect`` launch (or one replay of a graph that holds it)."""
        self.step += 1
        if self.step >= self.sweep_steps:
            self.step = 0
            self.sweep += 1

    def pair_sweep(self, distances: bool = False):
        """srwn_pair_sweep on the current stream, over the slot of the sweep the device has just completed; with
        `distances` the whole matrix goes to ``self.dist`` [N, N]."""
        import torch
        from . import kernels as K
        d, n = self.dataset, len(self.dataset)
        if self.emb is None:
            raise ValueError("embed_sampler: not bound to a model yet (bind)")
        if distances and self.dist is None:
            self.dist = torch.zeros((n, n), dtype=torch.float32, device=d.device)
        K.call("srwn_pair_sweep", self.emb.data_ptr(), d.labels.data_ptr(), self.state.data_ptr(), n, self.dim,
               self.sweep_capacity, self.bins, float(self.scale), self.nearest.data_ptr(), self.same_nearest.data_ptr(),
               self.rank_same.data_ptr(), self.nearest_dist.data_ptr(), self.same_dist.data_ptr(), self.hist_same.data_ptr(),
               self.hist_diff.data_ptr(), self.dist.data_ptr() if distances else None, K._stream())

    def result(self, sweep: int, step=None, distances: bool = False) -> "PairEvalResult":
        """Sweep number `sweep` (one of the last ``sweep_capacity`` completed) from its slot: the host waits here.  With
        `distances` the matrix of the last ``pair_sweep(distances=True)`` goes along."""
        sweep = int(sweep)
        if not max(0, self.sweep - self.sweep_capacity) <= sweep < self.sweep:
            raise ValueError("sweep %d: the slots hold sweeps [%d, %d)"
                             % (sweep, max(0, self.sweep - self.sweep_capacity), self.sweep))
        k = sweep % self.sweep_capacity
        host = lambda t: t[k].cpu().numpy()
        return PairEvalResult(host(self.emb), host(self.nearest), host(self.nearest_dist), host(self.same_nearest),
                              host(self.same_dist), host(self.rank_same), host(self.hist_same), host(self.hist_diff),
                              int(self.seen[k].item()), self.dataset._host_labels().astype(np.int32), self.bins, self.d_max,
                              step, self.dist.cpu().numpy() if distances and self.dist is not None else None)
