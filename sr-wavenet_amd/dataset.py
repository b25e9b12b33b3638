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

Storage is fp32 only: int16 or bf16 clip storage is out of scope.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

_MASK = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_CROP_SALT = 0x63726F706F666673
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

    def sampler(self, batch_size, num_samples, seed=0, shuffle=True, crop="head", rank=0, world=1, log_capacity=1024):
        return BatchSampler(self, batch_size, num_samples, seed, shuffle, crop, rank, world, log_capacity)


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class BatchSampler(object):
    """The draws of one training run on a ``DeviceDataset``.  Owns the device state ``{seed, step}`` (int64 [2]), the
    loss ring of ``log_capacity`` floats and the ``[batch_size]`` int32 indices of the last draw."""

    def __init__(self, dataset, batch_size, num_samples, seed=0, shuffle=True, crop="head", rank=0, world=1,
                 log_capacity=1024):
        batch_size, num_samples, rank, world = int(batch_size), int(num_samples), int(rank), int(world)
        _check_draw(batch_size, len(dataset), dataset.clip_len, num_samples, crop, rank, world)
        if int(log_capacity) < 1:
            raise ValueError("log_capacity %d: at least 1" % int(log_capacity))
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

    def seek(self, step: int) -> None:
        """Continues the sequence at `step` (a run resumed from a checkpoint): sets the device counter and the host's."""
        if int(step) < 0:
            raise ValueError("step %d" % int(step))
        self.state[1:].fill_(int(step))
        self.step = int(step)

    # ---- the two launches ------------------------------------------------------------------------------------------
    def draw(self, audio, audio2=None, codes=None, quantization_channels=0, onehot=None, onehot_rows=1, onehot_col0=0):
        """srwn_batch_draw on the current stream: the step's rows into `audio` ([B, T] fp32; `audio2` the same once
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
        K.call("srwn_batch_draw", d.audio.data_ptr(), None if d.labels is None else d.labels.data_ptr(), len(d),
               d.clip_len, self.state.data_ptr(), B, T, int(self.shuffle), CROPS[self.crop], self.rank, self.world, pa, pa2,
               pc, int(quantization_channels), po, ld, int(onehot_rows), int(onehot_col0), d.num_classes, odt,
               self.indices.data_ptr(), K._stream())

    def log_step(self, loss):
        """srwn_step_log on the current stream: ``log[step % log_capacity] = loss``, then the device step ticks."""
        import torch
        from . import kernels as K
        K.call("srwn_step_log", K._chk(loss, "loss", torch.float32, (1,)), self.log.data_ptr(), self.log_capacity,
               self.state.data_ptr(), K._stream())

    def losses(self, step0: int, count: int) -> np.ndarray:
        """The losses of steps [step0, step0 + count) from the ring (count <= log_capacity): the host waits here."""
        if not 0 <= count <= self.log_capacity:
            raise ValueError("the ring holds %d losses, asked for %d" % (self.log_capacity, count))
        ring = self.log.cpu().numpy()
        return ring[(step0 + np.arange(count)) % self.log_capacity].astype(np.float32)
