"""The deployable faces of the models of ``model.py``, NumPy in / NumPy out, with no training engine and no clip length:

* ``StreamingClassifier`` -- the ``WaveNet`` classifier on its own (recognizer.StreamClassifier).
* ``StreamingScorer``, ``StreamingMolScorer``, ``AutoEncoderScorer`` -- per-sample likelihoods (scorer.py).
* ``AudioEncoder``       -- the auto-encoder's encoder on its own (encoder.FrameEncoder): any batch, any length.
* ``GenerationPool``, ``LiveDecoding``, ``TeacherResynthesizer`` -- the autoregressive decoder as pools and live streams.
* ``StudentSynthesizer``, ``StudentInverter``, ``Resynthesizer`` -- the student's flows in both directions (student.py).
* ``StreamingEmbedder``  -- one ``SiameseWaveNet`` tower on its own (embedder.StreamEmbedder) with its gallery.

and their streams and pools; also the helpers both halves use (default dtype, conditions tiled onto frames, the flows'
variable names).  ``model.py`` imports this module; a face that needs a model class imports it inside the function."""
import os

import numpy as np
import torch

from . import kernels as K
from .engine import StackConfig
from .slots import SlotTable, per_stream, slot_list
from .training import _read_state


def _default_dtype():
    return torch.float32 if os.environ.get("SRWN_DTYPE", "bf16").lower() in ("f32", "fp32", "float32") else torch.bfloat16


# --- conditions ---------------------------------------------------------------------------------------------------
# The reference concatenates a clip's conditions onto every frame of its encoding (encoding_w_condition: model.py:161-167
# for the decoder, model.py:496-499 for the student's flows).
def _tile_conditions(frames, cond):
    """frames [B, k, latent] and conditions [B, condition_size] (torch, one device) -> [B, k, latent + condition_size]."""
    return torch.cat([frames, cond[:, None, :].expand(-1, frames.shape[1], -1)], dim=2)


def _tile_conditions_np(frames, cond):
    """One stream in NumPy: frames [k, latent] and conditions [1, condition_size] -> [k, latent + condition_size]."""
    return np.concatenate([frames, np.repeat(cond, frames.shape[0], 0)], 1)


def _check_conditions(batch, conditions, condition_size, who):
    """conditions as float32 NumPy [batch, condition_size] (None when the model `who` has none); no device work."""
    if condition_size <= 0:
        return None
    if conditions is None:
        raise ValueError("this %s was built with condition_size > 0; pass conditions [%d, %d]" % (who, batch, condition_size))
    c = np.asarray(conditions, dtype=np.float32)
    if c.shape != (batch, condition_size):
        raise ValueError("conditions must be [%d, %d]" % (batch, condition_size))
    return c


def _to_device(c):
    return None if c is None else torch.as_tensor(c).to("cuda")


def _device_conditions(batch, conditions, condition_size, who):
    """The same, checked and then on the device (the caller has asked for the GPU)."""
    return _to_device(_check_conditions(batch, conditions, condition_size, who))


class StreamingClassifier(object):
    """The deployable form of the ``WaveNet`` classifier (createNetwork, model.py:33-62) with a NumPy face: no training
    engine, no clip length.  ``classify(audio [B, T])`` -> probabilities [B, n_emit, C] of every window position
    (j + 1) * hop - window, j >= window / hop - 1, of a recording of any length; ``stream(batch)`` -> a
    ``ClassifierStream`` to ``push`` audio into as it arrives.  An emission does not depend on how the audio was cut."""

    def __init__(self, weights, max_batch=1, hop=160, window=16000, max_hops=8):
        from .recognizer import StreamClassifier
        self._w = weights
        self._eng = StreamClassifier(weights, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops)
        self.max_batch, self.hop, self.window = self._eng.max_batch, self._eng.hop, self._eng.window

    @classmethod
    def from_checkpoint(cls, logdir, dilations, output_channels, dilation_channels=32, skip_channels=256, filter_width=2,
                        name="WaveNet", dtype=None, max_batch=1, hop=160, window=16000, max_hops=8):
        """A classifier on the variables saved in `logdir` (``WaveNet.save``'s .pt form or a TensorFlow bundle, by the
        reference's variable names under `name`)."""
        from .recognizer import ClassifierWeights, check_classifier_widths, check_hop_window
        check_hop_window(hop, window)
        check_classifier_widths(filter_width, dilation_channels, skip_channels)
        w = ClassifierWeights(dilations, dilation_channels, skip_channels, output_channels, filter_width,
                              dtype or _default_dtype())
        if not w.load(logdir, name):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNet.save writes one)" % logdir)
        return cls(w, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops)

    def classify(self, inputs, return_logits=False):
        """inputs [B, T] -> probabilities [B, n_emit, C] (NumPy), n_emit = max(0, T // hop - window / hop + 1)."""
        out = self._eng.classify(self._eng._check_audio(inputs), return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()

    def stream(self, batch_size=1):
        return ClassifierStream(self, self._eng.start(batch_size))

    def pool(self, audio_ring=None):
        """A ``ClassifierPool``: this classifier's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio of any length at a clock of its own (``recognizer.ClassifierPool``).  audio_ring: samples a slot can hold
        (default 2 * max_hops * hop + 1).  Ends the current ``ClassifierStream``; ``stream`` and ``classify`` end the pool."""
        return ClassifierPool(self._eng.pool(audio_ring))


class ClassifierStream(object):
    """NumPy face of one running batch of classifier streams (``StreamingClassifier.stream``).  ``t``: samples received
    per stream; ``emitted``: emissions returned so far."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B

    @property
    def t(self):
        return self._st.t

    @property
    def emitted(self):
        return self._st.emitted

    def push(self, audio, return_logits=False):
        """audio [B, n], any n >= 0 -> probabilities [B, k, C] of the k window positions it completed (k may be 0)."""
        out = self._owner._eng.push(self._st, audio, return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()


class StreamingScorer(object):
    """The deployable likelihood scorer of the softmax ``WaveNetTeacher`` with a NumPy face: no training engine, no clip
    length.  ``score(audio [B, T])`` -> nll [B, T] in nats, nll[b, t] = -log p(mu_law_encode(audio)[b, t] | audio[b, < t]),
    for recordings of any length; ``stream(batch)`` -> a ``ScorerStream`` to ``push`` audio into as it arrives.  A value
    does not depend on how the audio was cut."""

    def __init__(self, weights, max_batch=1, max_chunk=1600):
        from .scorer import StreamScorer
        self._w = weights
        self._eng = StreamScorer(weights, max_batch=max_batch, max_chunk=max_chunk)
        self.max_batch, self.max_chunk = self._eng.max_batch, self._eng.max_chunk

    @classmethod
    def from_checkpoint(cls, logdir, dtype=None, max_batch=1, max_chunk=1600):
        """A scorer on the variables ``WaveNetTeacher.save`` left in `logdir` (its config.json names the stack; the
        checkpoint is this package's .pt form or a TensorFlow bundle, read by the reference's variable names)."""
        import json
        from types import SimpleNamespace
        from .recognizer import check_classifier_widths
        from .scorer import ScorerWeights
        path = os.path.join(logdir, "config.json")
        if not os.path.exists(path):
            raise FileNotFoundError("%s: no config.json (save the teacher with WaveNetTeacher.save)" % logdir)
        c = json.load(open(path))
        ScorerWeights.check_config(SimpleNamespace(
            head_mode="per_timestep" if c.get("head", "softmax") == "softmax" else "mol", gate_mode=c.get("gate_mode", "reference"),
            cond_channels=(c["latent_channels"] + c["condition_size"]) if c.get("use_encoding") else 0, shift_input=True))
        check_classifier_widths(c["filter_width"], c["dilation_channels"], c["skip_channels"], "streaming scorer")
        w = ScorerWeights(c["dilations"], c["dilation_channels"], c["skip_channels"], c["quantization_channels"],
                          c["filter_width"], dtype or _default_dtype())
        if not w.load(logdir, c.get("name", "WaveNetTeacher")):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNetTeacher.save writes one)" % logdir)
        return cls(w, max_batch=max_batch, max_chunk=max_chunk)

    @staticmethod
    def _numpy(out):
        return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()

    def score(self, inputs, return_logits=False, return_best=False):
        """inputs [B, T] -> nll [B, T] (NumPy, nats); with return_logits also the logits [B, T, C], with return_best also
        the most likely code [B, T]."""
        return self._numpy(self._eng.score(self._eng._check_audio(inputs), return_logits, return_best))

    def stream(self, batch_size=1):
        return ScorerStream(self, self._eng.start(batch_size))

    def pool(self, audio_ring=None):
        """A ``ScorerStreamPool``: this scorer's ``max_batch`` rows as slots that streams join and leave, each pushing audio
        of any length at a clock of its own (``scorer.ScorerPool``).  audio_ring: samples a slot can hold (default 2 *
        max_chunk + 2).  Ends the current ``ScorerStream``; ``stream`` and ``score`` end the pool."""
        return ScorerStreamPool(self._eng.pool(audio_ring))


class ScorerStream(object):
    """NumPy face of one running batch of scorer streams (``StreamingScorer.stream``).  ``t``: samples scored per
    stream."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B

    @property
    def t(self):
        return self._st.t

    def push(self, audio, return_logits=False, return_best=False):
        """audio [B, n], any n >= 0 -> nll [B, n] of exactly those samples."""
        return self._owner._numpy(self._owner._eng.push(self._st, audio, return_logits, return_best))

    def bits_per_sample(self):
        """Mean nll of everything pushed so far, in bits, per stream [B] (NaN before the first sample)."""
        from .scorer import bits_per_sample
        return np.array([bits_per_sample(v, self._st.t) for v in self._st.nll_sum.cpu().numpy()])


class _MolScorerFace(object):
    """What ``StreamingMolScorer`` and ``AutoEncoderScorer`` share: a ``scorer.MolStreamScorer`` ``_eng`` on a snapshot of
    decoder weights ``_w``, and the tiling of clip-level conditions onto encoding frames (``with_conditions``)."""

    def _setup(self, weights, latent_channels, condition_size, max_batch, max_chunk, max_frames):
        from .scorer import MolStreamScorer
        self._w = weights
        self.latent_channels, self.condition_size = int(latent_channels), int(condition_size)
        self._eng = MolStreamScorer(weights, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)
        self.max_batch, self.max_chunk, self.max_frames = self._eng.max_batch, self._eng.max_chunk, self._eng.max_frames
        self.pool_stride, self.conditioned = int(self._eng.pool), bool(self._eng.E)

    def _conditions(self, batch, conditions):
        """conditions [B, condition_size] on the device, or None (no device work before the refusals)."""
        if not self.conditioned:
            if conditions is not None:
                raise ValueError("this decoder is not conditioned")
            return None
        c = _check_conditions(batch, conditions, self.condition_size, "scorer")
        return None if c is None else torch.as_tensor(c, device="cuda")

    def _frames(self, encoding, cond):
        """encoding [B, k, latent] (NumPy or device) -> the conditioning frames [B, k, latent + condition_size] (device)."""
        e = torch.as_tensor(encoding, dtype=torch.float32)
        if e.dim() != 3 or e.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels=%d], got %s"
                             % (self.latent_channels, tuple(e.shape)))
        e = e.to("cuda")
        return e if cond is None else _tile_conditions(e, cond)

    def _score(self, inputs, encoding, conditions, return_logits):
        x = self._eng._check_audio(inputs)
        enc = None
        if self.conditioned:
            if encoding is None:
                raise ValueError("this decoder is conditioned: pass encoding [batch, samples / pool_stride, %d]"
                                 % self.latent_channels)
            enc = self._frames(encoding, self._conditions(int(x.shape[0]), conditions))
        elif encoding is not None or conditions is not None:
            raise ValueError("this decoder is not conditioned")
        out = self._eng.score(x, enc, return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()


class _MolScoreStreamBase(object):
    """NumPy face of one running batch of mixture-of-logistics scorer streams.  ``t``: samples scored per stream."""

    def __init__(self, owner, batch_size, conditions):
        self._owner, self.batch_size = owner, int(batch_size)
        self._cond = owner._conditions(self.batch_size, conditions)      # (its refusals come before any device work)
        self._st = owner._eng.start(self.batch_size)

    t = property(lambda self: self._st.t)
    fed = property(lambda self: self._st.fed)

    def bits_per_sample(self):
        """Mean nll of everything scored so far, in bits, per stream [B] (NaN before the first sample)."""
        from .scorer import bits_per_sample
        return np.array([bits_per_sample(v, self._st.t) for v in self._st.nll_sum.cpu().numpy()])


class StreamingMolScorer(_MolScorerFace):
    """The deployable likelihood scorer of the mixture-of-logistics ``WaveNetTeacher`` (the model the student distils
    from), conditioned or not, with a NumPy face: ``score(inputs [B, T], encoding, conditions)`` -> nll [B, T] in nats,
    nll[b, t] = -log p(inputs[b, t] | inputs[b, < t], encoding); ``stream(batch, conditions)`` -> a ``MolScorerStream`` to
    ``feed`` frames and ``push`` audio into as they arrive.  A value does not depend on how audio and frames were cut."""

    def __init__(self, weights, latent_channels=0, condition_size=0, max_batch=1, max_chunk=1600, max_frames=32):
        self._setup(weights, latent_channels, condition_size, max_batch, max_chunk, max_frames)

    def score(self, inputs, encoding=None, conditions=None, return_logits=False):
        """inputs [B, T] (T = frames * pool_stride for a conditioned teacher) -> nll [B, T] (NumPy, nats); with
        return_logits also the logits [B, T, 4 * num_mixtures]."""
        return self._score(inputs, encoding, conditions, return_logits)

    def stream(self, batch_size=1, conditions=None):
        return MolScorerStream(self, batch_size, conditions)

    def pool(self, audio_ring=None):
        """A ``MolScorerStreamPool``: this scorer's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio and being fed frames at a clock of its own (``scorer.MolScorerPool``).  audio_ring: samples a slot can hold
        (default 2 * max_chunk + 2).  Ends the current ``MolScorerStream``; ``stream`` and ``score`` end the pool."""
        return MolScorerStreamPool(self, self._eng.pool(audio_ring))


class MolScorerStream(_MolScoreStreamBase):
    """``StreamingMolScorer.stream``: ``feed(encoding [B, k, latent])`` hands every stream its next k <= ``room`` frames,
    ``push(audio [B, n])`` scores the next n <= ``available`` samples (an unconditioned teacher: any n, nothing to feed)."""

    room = property(lambda self: self._owner._eng.room(self._st))
    available = property(lambda self: self._owner._eng.available(self._st))

    def feed(self, encoding):
        if not self._owner.conditioned:
            raise ValueError("feed: this teacher is not conditioned")
        self._owner._eng.feed(self._st, self._owner._frames(encoding, self._cond))

    def push(self, audio, return_logits=False):
        out = self._owner._eng.push(self._st, audio, return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()


class AutoEncoderScorer(_MolScorerFace):
    """The whole ``WaveNetAutoEncoder`` as a likelihood meter: an ``AudioEncoder`` (a snapshot of the encoder) feeding a
    ``scorer.MolStreamScorer`` on a snapshot of the decoder -- audio in, nll[b, t] = -log p(audio[b, t] | audio[b, < t],
    encode(audio)) in nats out, the number the auto-encoder is trained on, for recordings of any length.  ``score`` scores
    the (T // pool_stride) * pool_stride samples whose frames exist; ``stream`` does so as the audio arrives, a sample as
    soon as the encoder has completed its frame, with the same bits however the audio was cut."""

    def __init__(self, encoder, weights, condition_size=0, max_batch=1, max_chunk=1600, max_frames=32):
        if not isinstance(encoder, AudioEncoder):
            raise TypeError("AutoEncoderScorer(encoder: AudioEncoder, weights: scorer.MolScorerWeights)")
        if int(encoder.pool_stride) != int(weights.pool) or weights.E != encoder.latent_channels + int(condition_size):
            raise ValueError("the encoder gives %d-channel frames per %d samples, the decoder takes %d channels (%d of "
                             "them conditions) per %d" % (encoder.latent_channels, encoder.pool_stride, weights.E,
                                                          int(condition_size), weights.pool))
        self.encoder = encoder
        self._setup(weights, encoder.latent_channels, condition_size, max_batch, max_chunk, max_frames)

    @classmethod
    def from_checkpoint(cls, logdir, dtype=None, max_batch=1, max_chunk=1600, max_frames=32):
        """A scorer on the variables ``WaveNetAutoEncoder.save`` left in `logdir` (its config.json names both halves)."""
        import json
        from .scorer import MolScorerWeights
        path = os.path.join(logdir, "config.json")
        if not os.path.exists(path):
            raise FileNotFoundError("%s: no config.json (save the model with WaveNetAutoEncoder.save)" % logdir)
        c = json.load(open(path))
        dt = dtype or _default_dtype()
        enc = AudioEncoder.from_checkpoint(logdir, dtype=dt, max_batch=max_batch, max_frames=max_frames)
        w = MolScorerWeights(c["dilations"], c["dilation_channels"], c["skip_channels"], c["num_mixtures"],
                             c["latent_channels"] + c["condition_size"], c["pool_stride"], c["filter_width"], dt)
        if not w.load(logdir, c.get("name", "WaveNetAutoEncoder") + "/Decoder"):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNetAutoEncoder.save writes one)" % logdir)
        return cls(enc, w, c["condition_size"], max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)

    def score_with_encoding(self, inputs, encoding, conditions=None, return_logits=False):
        """inputs [B, frames * pool_stride], encoding [B, frames, latent_channels] -> nll (NumPy, nats)."""
        return self._score(inputs, encoding, conditions, return_logits)

    def score(self, inputs, conditions=None, return_logits=False):
        """inputs [B, T] of any T -> nll [B, (T // pool_stride) * pool_stride] under the encoding of the inputs."""
        x = self.encoder._check(inputs)
        enc = self.encoder._eng.encode(torch.as_tensor(x))
        return self._score(x[:, :int(enc.shape[1]) * self.pool_stride], enc, conditions, return_logits)

    def stream(self, batch_size=1, conditions=None):
        if not 1 <= int(batch_size) <= min(self.max_batch, self.encoder.max_batch):
            raise ValueError("batch_size %r: this scorer holds %d streams" % (batch_size, min(self.max_batch, self.encoder.max_batch)))
        return AutoEncoderScoreStream(self, int(batch_size), conditions)

    def pool(self, audio_ring=None):
        """An ``AutoEncoderScorerPool``: an encoder pool feeding a scorer pool, slot by slot, each stream at a clock of its
        own.  audio_ring: samples a slot of the SCORER half can hold (default: the encoder pool's ring plus max_chunk + 2;
        at least ``scorer.ae_pool_min_audio_ring``).  Ends the current stream of either half."""
        return AutoEncoderScorerPool(self, audio_ring)


class AutoEncoderScoreStream(_MolScoreStreamBase):
    """``AutoEncoderScorer.stream``: ``push(audio [B, n])``, any n, returns the nll of every sample whose frame the encoder
    has completed by now ([B, m], m >= 0); audio that cannot be scored yet waits on the device.  ``finish()`` returns the
    rest (the encoder's last whole frames, with its clip-end padding) and closes the stream.  ``received``: samples
    pushed; ``t``: samples scored."""

    def __init__(self, owner, batch_size, conditions):
        super().__init__(owner, batch_size, conditions)
        self._enc = owner.encoder._eng.start(self.batch_size)
        self._backlog = torch.zeros((self.batch_size, 0), dtype=torch.float32, device="cuda")

    received = property(lambda self: self._enc.received)

    def _drain(self, frames):
        """frames [B, k, latent] (device) into the ring and every sample they allow: feed -> push -> feed while the ring
        has less room than the frames that are due."""
        o, st, outs = self._owner, self._st, []
        eng, k, f0 = o._eng, int(frames.shape[1]), 0
        while True:
            if f0 < k:
                r = min(eng.room(st), k - f0)
                if r > 0:
                    eng.feed(st, o._frames(frames[:, f0:f0 + r], self._cond))
                    f0 += r
            n = int(eng.available(st))
            if n <= 0:
                if f0 < k:      # (cannot happen: max_frames >= live_min_frames leaves room once every sample is scored)
                    raise RuntimeError("the conditioning ring has no room and no sample to score")
                break
            outs.append(eng.push(st, self._backlog[:, :n]))
            self._backlog = self._backlog[:, n:]
        if not outs:
            return np.zeros((self.batch_size, 0), np.float32)
        return torch.cat(outs, dim=1).cpu().numpy()

    def push(self, audio):
        if self._enc.closed:
            raise ValueError("this stream is closed (finish was called)")
        x = torch.as_tensor(self._owner.encoder._check(audio, self.batch_size))
        frames = self._owner.encoder._eng.push(self._enc, x)
        self._backlog = torch.cat([self._backlog, x.to("cuda")], dim=1)
        return self._drain(frames)

    def finish(self):
        out = self._drain(self._owner.encoder._eng.finish(self._enc))
        self._backlog = self._backlog[:, :0]
        return out


def _pool_encodings(n, encoding, conditions, latent, condition_size):
    """The per-stream encodings of a pool join: n of [frames_i, latent] (+ conditions [condition_size] tiled over the
    frames) -> n float32 arrays [frames_i, latent + condition_size]."""
    if encoding is None:
        raise ValueError("this decoder is conditioned: pass encoding, one [frames, latent] per stream")
    encs = per_stream(encoding, n, "encodings")
    conds = per_stream(conditions, n, "conditions")
    out = []
    for e, c in zip(encs, conds):
        e = np.asarray(e, dtype=np.float32)
        if e.ndim != 2 or e.shape[1] != latent:
            raise ValueError("join: each encoding is [frames, %d], got shape %s" % (latent, e.shape))
        if condition_size > 0:
            if c is None:
                raise ValueError("built with condition_size > 0: pass conditions, one [%d] per stream" % condition_size)
            e = _tile_conditions_np(e, np.asarray(c, dtype=np.float32).reshape(1, condition_size))
        out.append(e)
    return out


def _check_prompt(batch_size, prompt):
    if prompt is None:
        return None
    p = np.asarray(prompt, dtype=np.float32)
    if p.ndim != 2 or p.shape[0] != int(batch_size):
        raise ValueError("prompt must be [batch=%d, P], got shape %s" % (int(batch_size), p.shape))
    return p


def _stream_chunks(eng, st, chunk, mode, max_samples):
    """The blocks of a primed generation state (WaveNetEngine.generate_chunk) until max_samples or the encoding ends."""
    made = 0
    while True:
        n = chunk
        if max_samples is not None:
            n = min(n, int(max_samples) - made)
        if st.limit is not None:
            n = min(n, st.limit - st.t)
        if n <= 0:
            return
        a, _, _ = eng.generate_chunk(st, n, mode=mode)
        made += n
        yield a.cpu().numpy()


def _ran_dict(a, ran, slots):
    """A pool step's device rows a [capacity, n] as {slot: its ran[slot] samples} (NumPy) for the `slots` that made some."""
    a = a.cpu().numpy()
    return {u: a[u, :int(ran[u])] for u in slots if ran[u] > 0}


def _host_dict(d):
    """A pool step's {slot: device rows} as {slot: NumPy rows}, with ONE device-to-host copy however many slots."""
    us = list(d)
    if len(us) < 2:
        return {u: d[u].cpu().numpy() for u in us}
    flat = torch.cat([d[u] for u in us], dim=0).cpu().numpy()
    return dict(zip(us, np.split(flat, np.cumsum([d[u].shape[0] for u in us])[:-1])))


def _audio_pieces(slots, audio):
    """What a pool's ``push`` was given as one array per slot: one slot, or one 1-D array, is a single piece."""
    one = np.isscalar(slots) or (isinstance(audio, np.ndarray) and audio.dtype != object and audio.ndim == 1)
    return [np.asarray(a) for a in ([audio] if one else audio)]


class _PoolFace(object):
    """What the NumPy faces of the pools share: ``self._pool``'s slot view, forwarded."""

    capacity = property(lambda self: self._pool.capacity)
    active = property(lambda self: self._pool.active)
    free = property(lambda self: self._pool.free)

    def leave(self, slots):
        self._pool.leave(slots)


class GenerationPool(_PoolFace):
    """NumPy face of a generation pool (engine.GenerationPool): a fixed number of slots over one set of rings that streams
    join and leave while it runs.  ``join(seed=[...], prompt=[...], ...)`` takes one entry per stream and returns their
    slots; ``step(n)`` runs n pool steps in one launch and returns ``{slot: samples}`` of every slot that produced some; a
    stream that reaches its end frees its slot; ``leave(slots)`` ends streams early.  A stream's samples put together are
    what a batch-of-one ``generate`` with its seed and prompt returns.  On a live pool
    (``WaveNetAutoEncoder.generation_pool(..., live=True)``) ``join(..., live=True)`` / ``feed`` / ``room`` / ``close``
    mirror ``SynthesisPool``: the stream is fed while it runs and waits, with no samples, while it has none to make."""

    def __init__(self, pool, cond_fn, mode, latent=None, condition_size=0):
        self._pool, self._cond_fn, self.mode = pool, cond_fn, mode
        self._latent, self._cs = latent, int(condition_size)
        self._live_cond = {}      # slot -> the conditions of the live stream joined there last

    t = property(lambda self: self._pool.t)

    def join(self, seed, prompt=None, encoding=None, conditions=None, max_samples=None, *, temperature=None, top_k=None,
             top_p=None, live=False):
        """temperature / top_k / top_p: the joining streams' sampling controls (a scalar or one entry per stream; None = the
        default), as `generate` takes them.  encoding: one [frames_i, latent] per stream.
        live=True (a live pool): a single 2-D array is one stream; an encoding holds a stream's first frames ([0, latent]: none yet), its conditions are kept
        and tiled onto every frame fed later (``feed``); a live stream that has used up its frames waits (no samples)
        until it is fed, closed or left."""
        if live:
            K._need_gpu()
        if live and isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
            conditions = None if conditions is None else [conditions]
        seeds = [int(s) for s in (seed if np.ndim(seed) else [seed])]
        n = len(seeds)
        prompts = per_stream(prompt, n, "prompts")
        for p in prompts:
            if p is not None and np.ndim(p) != 1:
                raise ValueError("join: each prompt is 1-D [P], got shape %s" % (np.shape(p),))
        prompts = [None if p is None else np.asarray(p, dtype=np.float32) for p in prompts]
        mx = per_stream(max_samples, n, "max_samples")
        cond = self._cond_fn(n, encoding, conditions)
        if live:
            slots = self._pool.join(seeds, prompts, cond, mx, temperature=temperature, top_k=top_k, top_p=top_p, live=True)
            if self._cs > 0:
                for u, c in zip(slots, per_stream(conditions, n, "conditions")):
                    self._live_cond[u] = np.asarray(c, dtype=np.float32).reshape(1, self._cs)
            return slots
        if temperature is None and top_k is None and top_p is None:
            return self._pool.join(seeds, prompts, cond, mx)
        return self._pool.join(seeds, prompts, cond, mx, temperature=temperature, top_k=top_k, top_p=top_p)

    def feed(self, slots, encoding):
        """The next frames of live slots: encoding[i] [k_i, latent] for slots[i] (k_i <= ``room``)."""
        slots = slot_list(slots, self.capacity, "feed")
        if isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
        encs = [np.asarray(e, dtype=np.float32) for e in encoding]
        if len(encs) != len(slots):
            raise ValueError("feed: %d slots but %d encodings" % (len(slots), len(encs)))
        for e in encs:
            if e.ndim != 2 or e.shape[1] != self._latent:
                raise ValueError("feed: each encoding is [k, %s], got shape %s" % (self._latent, e.shape))
        if self._cs > 0:
            if any(u not in self._live_cond for u in slots):
                raise ValueError("feed: slots %s are not all live streams of this pool" % (slots,))
            encs = [_tile_conditions_np(e, self._live_cond[u]) for u, e in zip(slots, encs)]
        self._pool.feed(slots, encs)

    def room(self, slot):
        return self._pool.room(int(slot))

    def close(self, slots):
        """No more frames will come for these live streams: each frees its slot at the end of what it was fed."""
        self._pool.close(slots)

    def step(self, n, mode=None, forced=None):
        a, _, _, ran = self._pool.step(int(n), mode=mode or self.mode, forced=forced)
        return _ran_dict(a, ran, range(self._pool.capacity))


class _LiveStream(object):
    """What ``LiveDecoding`` and ``LiveSynthesis`` share: a running batch of ``batch_size`` streams of ``_owner`` on the
    engine state ``_st``, fed through a conditioning ring of ``_ring`` frames, with the conditions ``_cond`` (device, or
    None) tiled onto every frame fed.  A subclass gives ``room``, ``_take`` (the engine call the frames go to) and
    ``step`` / ``_step_device``."""

    def __init__(self, owner, state, cond, batch, ring):
        self._owner, self._st, self._cond, self.batch_size, self._ring = owner, state, cond, batch, ring

    t = property(lambda self: self._st.t)
    fed = property(lambda self: self._st.fed)

    @property
    def available(self):
        """Samples that can be made now: fed * pool_stride - t."""
        return self._st.limit - self._st.t

    def _feed_device(self, enc):
        """enc [B, k, latent] on the device (or NumPy): + the tiled conditions, into the ring."""
        o = self._owner
        e = torch.as_tensor(enc, dtype=torch.float32)
        if e.dim() != 3 or e.shape[0] != self.batch_size or e.shape[2] != o.latent_channels:
            raise ValueError("encoding must be [%d, k, latent_channels=%d], got %s"
                             % (self.batch_size, o.latent_channels, tuple(e.shape)))
        if e.shape[1] > self.room:
            raise ValueError("feed: %d frames, but the ring of %d has room for %d at t = %d with %d fed"
                             % (e.shape[1], self._ring, self.room, self.t, self.fed))
        if self._cond is not None:
            e = _tile_conditions(e.to("cuda"), self._cond)
        self._take(e)

    def feed(self, encoding):
        self._feed_device(encoding if isinstance(encoding, torch.Tensor) else np.asarray(encoding, dtype=np.float32))


class LiveDecoding(_LiveStream):
    """One running batch of live decoder streams (``WaveNetAutoEncoder.live``).  ``feed(encoding [B, k, latent])`` hands
    every stream its next k frames (k <= ``room``), ``step(n)`` returns the next n <= ``available`` samples [B, n]; ``t``:
    samples made so far (a prompt's included), ``fed``: frames fed.  The samples are those ``generate`` gives the whole
    encoding with the same seed and temperature, however the frames and chunks were cut."""

    def __init__(self, owner, dec, state, cond, mode):
        super().__init__(owner, state, cond, state.batch, state.max_frames)
        self._dec, self._mode = dec, mode

    @property
    def room(self):
        from .engine import live_decode_room
        return live_decode_room(self._st.max_frames, self._st.fed, self._st.t, self._owner.pool_stride)

    def _take(self, e):
        self._dec.feed(self._st, e)

    def _step_device(self, n, forced=None, want_logits=False):
        """(audio [B, n] f32, selected mixture [B, n] i32, logits [B, n, 4M] f32 or None) on the device."""
        return self._dec.generate_chunk(self._st, int(n), mode=self._mode, forced=forced, want_logits=want_logits)

    def step(self, n, forced=None, return_logits=False):
        """The next n samples [B, n] (NumPy); forced [B, n]: teacher forcing for this chunk; return_logits: (samples, logits
        [B, n, 4 * num_mixtures])."""
        a, _, lg = self._step_device(n, forced, return_logits)
        return (a.cpu().numpy(), lg.cpu().numpy()) if return_logits else a.cpu().numpy()


def _check_resynthesis_halves(who, encoder, other, other_type, arg, half):
    """What both resynthesizers ask of their halves -- an ``AudioEncoder`` and `other` (the argument `arg`, of
    `other_type`, whose `half` reads the frames) with one pool_stride and one latent width.  Returns ``lookahead``: the
    samples of audio a sample of output waits for beyond itself, the rest of its frame and the encoder's look-ahead."""
    if not isinstance(encoder, AudioEncoder) or not isinstance(other, other_type):
        raise TypeError("%s(encoder: AudioEncoder, %s: %s)" % (who, arg, other_type.__name__))
    if int(encoder.pool_stride) != int(other.pool_stride):
        raise ValueError("pool_stride: the encoder makes a frame per %d samples, the %s reads one per %d"
                         % (encoder.pool_stride, half, other.pool_stride))
    if int(encoder.latent_channels) != int(other.latent_channels):
        raise ValueError("latent_channels: the encoder gives %d, the %s takes %d"
                         % (encoder.latent_channels, half, other.latent_channels))
    return int(encoder.pool_stride) + encoder.num_layers + 1


class _ResynthesisStream(object):
    """One running batch of a resynthesizer's ``stream``: an encoder stream state ``_enc`` whose frames go, on the device,
    into the live half ``_live`` (a ``_LiveStream``).  ``t``: samples returned so far per stream; ``received``: samples
    pushed.  ``push`` may return no sample while the first frame's look-ahead is incomplete.  A subclass gives
    ``_start_live``, ``_audio`` (the audio of what its live half's ``_step_device`` returns) and ``_tail``, the axes its
    results have after [B, m]."""

    _tail = ()

    def __init__(self, owner, batch, conditions, seed, temperature, chunk_size):
        self._owner, self.batch_size, self._chunk = owner, batch, chunk_size
        self._live = self._start_live(batch, conditions, seed, temperature)      # (its refusals come before any device work)
        self._enc = owner.encoder._eng.start(batch)

    t = property(lambda self: self._live.t)
    received = property(lambda self: self._enc.received)

    def _audio(self, chunk):
        return chunk

    def _drain(self, frames, outs):
        """frames [B, k, latent] (device) into the ring and every sample they allow: feed -> step -> feed while the ring
        has less room than the frames that are due."""
        live, k, f0 = self._live, int(frames.shape[1]), 0
        while True:
            if f0 < k:
                r = min(live.room, k - f0)
                if r > 0:
                    live._feed_device(frames[:, f0:f0 + r])
                    f0 += r
            n = min(live.available, self._chunk)
            if n <= 0:
                if f0 < k:      # (cannot happen on a ring that starts a live stream: room > 0 once every sample is made)
                    raise RuntimeError("the conditioning ring has no room and no sample to make")
                return
            outs.append(self._audio(live._step_device(n)))

    def _result(self, outs):
        B = self.batch_size
        if not outs:
            return np.zeros((B, 0) + self._tail, np.float32)
        return torch.cat(outs, dim=1).view(B, -1, *self._tail).cpu().numpy()

    def push(self, audio):
        if self._enc.closed:
            raise ValueError("this stream is closed (finish was called)")
        x = self._owner.encoder._check(audio, self.batch_size)
        outs = []
        self._drain(self._owner.encoder._eng.push(self._enc, torch.as_tensor(x)), outs)
        return self._result(outs)

    def finish(self):
        """The encoder's remaining whole frames (clip-end padding) and the samples they allow; closes the stream."""
        outs = []
        self._drain(self._owner.encoder._eng.finish(self._enc), outs)
        return self._result(outs)


class TeacherResynthesizer(object):
    """The live auto-encoder loop at teacher quality: an ``AudioEncoder`` feeding the autoregressive decoder of a
    ``WaveNetAutoEncoder`` (``Resynthesizer`` is the same pipeline on the student).  Audio chunks in, decoded audio chunks
    out, with no bound on the length; the latent frames go from the encoder into the decoder's conditioning ring as device
    tensors.  The audio of a stream put together equals ``autoencoder.generate(encoder.encode(audio), conditions,
    seed=seed, ...)`` however the audio and the chunks were cut."""

    def __init__(self, encoder, autoencoder, max_frames=None):
        from .model import WaveNetAutoEncoder
        self.lookahead = _check_resynthesis_halves("TeacherResynthesizer", encoder, autoencoder, WaveNetAutoEncoder,
                                                   "autoencoder", "decoder")
        K._need_gpu()
        self.encoder, self.autoencoder = encoder, autoencoder
        self.pool_stride = int(encoder.pool_stride)
        self.max_frames = int(max_frames if max_frames is not None else encoder.max_frames)

    def stream(self, batch=1, conditions=None, seed=0, temperature=1.0, chunk_size=160):
        """A ``TeacherResynthesisStream`` of `batch` streams in lockstep: ``push(audio [B, m])`` returns every sample that
        can be made by now, [B, m']; ``finish()`` the rest.  conditions [B, condition_size] are tiled onto every frame on
        the device; chunk_size: the most samples of one decoder launch."""
        batch, chunk_size = int(batch), int(chunk_size)
        if not 1 <= batch <= self.encoder.max_batch:
            raise ValueError("batch %d: the encoder holds %d streams" % (batch, self.encoder.max_batch))
        if chunk_size < 1:
            raise ValueError("chunk_size %d: at least 1" % chunk_size)
        return TeacherResynthesisStream(self, batch, conditions, seed, temperature, chunk_size)

    def pool(self, chunk_size=160, audio_ring=None):
        """A ``TeacherResynthesisPool``: independent callers on one encoder and one decoder.  Streams join and leave while
        the batch runs, audio arrives ragged, and each caller receives what it would have received alone.  chunk_size: the
        samples a ``step`` makes per stream at most; audio_ring: samples of audio a slot can hold (``AudioEncoder.pool``)."""
        K._need_gpu()
        return TeacherResynthesisPool(self, int(chunk_size), audio_ring)


class TeacherResynthesisStream(_ResynthesisStream):
    """One running batch of ``TeacherResynthesizer.stream``: ``push`` / ``finish`` return samples [B, m]."""

    def _start_live(self, batch, conditions, seed, temperature):
        o = self._owner
        return o.autoencoder.live(batch, conditions, o.max_frames, seed=seed, temperature=temperature)

    def _audio(self, chunk):
        return chunk[0]      # of (audio, selected mixture, logits)


class AudioEncoder(object):
    """The deployable form of the auto-encoder's encoder (createEncoder, model.py:136-156): audio in, latent frames out
    (``encoder.FrameEncoder``), with no decoder and no training state anywhere.  One object serves any batch <=
    ``max_batch`` and any length, whole clips (``encode``) or chunk by chunk (``stream``); a frame's value does not
    depend on how the audio was cut.  ``load`` reads what ``WaveNetAutoEncoder.save`` wrote, by the reference's
    variable names; the decoder's variables in the file are ignored."""

    def __init__(self, num_layers, skip_channels=256, latent_channels=16, pool_stride=512, encoder_channels=128,
                 filter_width=2, name="WaveNetAutoEncoder", dtype=None, max_batch=1, max_frames=32):
        from .encoder import EncoderWeights, FrameEncoder, _check_encoder_widths
        _check_encoder_widths(encoder_channels, filter_width, skip_channels)
        K._need_gpu()
        self.num_layers, self.skip_channels, self.latent_channels = int(num_layers), skip_channels, latent_channels
        self.pool_stride, self.encoder_channels, self.filter_width = int(pool_stride), encoder_channels, filter_width
        self._name = name
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        self._w = EncoderWeights(self.num_layers, encoder_channels, skip_channels, latent_channels, filter_width,
                                 dtype or _default_dtype())
        self._eng = FrameEncoder(self._w, self.pool_stride, max_batch=max_batch, max_frames=max_frames)

    @property
    def network_params(self):
        return self._w.tf_variables(self._name + "/Encoder")

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._w.repack()
        return ok

    @classmethod
    def from_checkpoint(cls, logdir, **kwargs):
        """An encoder on the variables saved in `logdir`, with the hyper-parameters of the ``config.json`` that
        ``WaveNetAutoEncoder.save`` writes beside them; kwargs: dtype, max_batch, max_frames."""
        import json
        with open(os.path.join(logdir, "config.json")) as f:
            cfg = json.load(f)
        enc = cls(len(cfg["dilations"]), skip_channels=cfg["skip_channels"], latent_channels=cfg["latent_channels"],
                  pool_stride=cfg["pool_stride"], encoder_channels=cfg["encoder_channels"],
                  filter_width=cfg["filter_width"], name=cfg.get("name", "WaveNetAutoEncoder"), **kwargs)
        if not enc.load(logdir):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNetAutoEncoder.save writes one)" % logdir)
        return enc

    def _check(self, inputs, batch=None):
        """Shape refusals, before anything touches the device."""
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("inputs must be [batch, samples], got shape %s" % (x.shape,))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError("batch %d: this encoder was built for max_batch=%d" % (x.shape[0], self.max_batch))
        if batch is not None and x.shape[0] != batch:
            raise ValueError("audio of %d streams pushed into a stream of %d" % (x.shape[0], batch))
        return x

    def encode(self, inputs):
        """inputs [B, T] -> encoding [B, T // pool_stride, latent_channels] (NumPy), for any T."""
        x = self._check(inputs)
        return self._eng.encode(torch.as_tensor(x)).cpu().numpy()

    def stream(self, batch_size=1):
        """An ``EncoderStream`` of `batch_size` streams in lockstep: ``push(audio [B, n])`` returns the frames whose
        look-ahead is complete, ``finish()`` the rest with the clip-end padding."""
        if not 1 <= int(batch_size) <= self.max_batch:
            raise ValueError("batch_size %r: this encoder was built for max_batch=%d" % (batch_size, self.max_batch))
        return EncoderStream(self, int(batch_size))

    def pool(self, audio_ring=None, max_rows=None):
        """An ``AudioEncoderPool``: this encoder's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio of any length at a clock of its own (``encoder.EncoderPool``).  audio_ring: samples a slot can hold
        (default max_frames * pool_stride + num_layers + 1 + pool_stride); max_rows: frames per launch."""
        K._need_gpu()
        return AudioEncoderPool(self._eng.pool(audio_ring, max_rows))


class EncoderStream(object):
    """NumPy face of one running batch of encoder streams (``AudioEncoder.stream``).  ``t``: samples received per
    stream; ``frames``: frames emitted.  Everything ``push`` returned followed by what ``finish`` returns equals
    ``AudioEncoder.encode`` of the concatenated audio."""

    def __init__(self, owner, batch_size):
        self._owner, self.batch_size = owner, batch_size
        self._st = owner._eng.start(batch_size)

    @property
    def t(self):
        return self._st.received

    @property
    def frames(self):
        return self._st.emitted

    def push(self, audio):
        if self._st.closed:
            raise ValueError("this stream is closed (finish was called)")
        x = self._owner._check(audio, self.batch_size)
        return self._owner._eng.push(self._st, torch.as_tensor(x)).cpu().numpy()

    def finish(self):
        return self._owner._eng.finish(self._st).cpu().numpy()


class _AudioPoolFace(_PoolFace):
    """What the NumPy faces of the pools that take audio share (``self._pool``: an ``audio_ring.AudioRingSlots``)."""

    def __init__(self, pool):
        self._pool = pool

    received = property(lambda self: self._pool.received)
    emitted = property(lambda self: self._pool.emitted)

    def audio_room(self, slot):
        return self._pool.audio_room(int(slot))

    def join(self, n=1, slots=None):
        return self._pool.join(n, slots)

    def push(self, slots, audio):
        self._pool.push([int(slots)] if np.isscalar(slots) else slots, _audio_pieces(slots, audio))


class AudioEncoderPool(_AudioPoolFace):
    """NumPy face of an encoder pool (``AudioEncoder.pool``; encoder.EncoderPool).  ``join`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``finish(slots)`` ends streams, ``step()`` returns
    ``{slot: frames [k, latent]}`` for every slot with new frames and frees the finished slots whose frames are all out.
    A stream's frames put together are ``AudioEncoder.encode`` of its audio alone."""

    def finish(self, slots):
        self._pool.finish(slots)

    def step(self, limit=None):
        return {u: f.cpu().numpy() for u, f in self._pool.step(limit).items()}


class ClassifierPool(_AudioPoolFace):
    """NumPy face of a classifier pool (``StreamingClassifier.pool``; recognizer.ClassifierPool).  ``join`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``step()`` returns ``{slot: probabilities [e, C]}``
    for every slot whose stream completed window positions (with return_logits a second dict with the pooled logits).  A
    stream's emissions put together are ``StreamingClassifier.classify`` of its audio alone."""

    audio_ring = property(lambda self: self._pool.audio_ring)
    consumed = property(lambda self: self._pool.consumed)

    def step(self, return_logits=False):
        out = self._pool.step(return_logits)
        host = lambda d: {u: f.cpu().numpy() for u, f in d.items()}
        return (host(out[0]), host(out[1])) if return_logits else host(out)


class ScorerStreamPool(_AudioPoolFace):
    """NumPy face of a scorer pool (``StreamingScorer.pool``; scorer.ScorerPool).  ``join`` returns slots, ``push(slots,
    audio)`` takes one 1-D array per slot, of any length, ``step()`` returns ``{slot: nll [m]}`` (nats) for every slot whose
    stream scored m > 0 samples (with return_logits / return_best further dicts, in that order).  A stream's nll put
    together is ``StreamingScorer.score`` of its audio alone."""

    audio_ring = property(lambda self: self._pool.audio_ring)
    scored = property(lambda self: self._pool.scored)
    nll_sum = property(lambda self: self._pool.nll_sum)

    def bits_per_sample(self, slot):
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        return self._pool.bits_per_sample(int(slot))

    def step(self, return_logits=False, return_best=False):
        out = self._pool.step(return_logits, return_best)
        host = lambda d: {u: f.cpu().numpy() for u, f in d.items()}
        return tuple(host(d) for d in out) if isinstance(out, tuple) else host(out)


class MolScorerStreamPool(_AudioPoolFace):
    """NumPy face of a mixture-of-logistics scorer pool (``StreamingMolScorer.pool``; scorer.MolScorerPool).
    ``join(conditions, n)`` returns slots (conditions [n, condition_size], one row per stream, tiled onto every frame the
    stream is fed), ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``feed(slots, encoding)`` one
    [k, latent_channels] array per slot with k <= ``room(slot)``, ``step()`` returns ``{slot: nll [m]}`` (nats) for every slot
    whose stream scored m > 0 samples (with return_logits a second dict).  A stream's nll put together is
    ``StreamingMolScorer.score`` of its audio and encoding alone."""

    def __init__(self, owner, pool):
        super().__init__(pool)
        self._owner, self._cond = owner, {}      # slot -> its stream's conditions [1, condition_size] on the device, or None

    audio_ring = property(lambda self: self._pool.audio_ring)
    scored = property(lambda self: self._pool.scored)
    fed = property(lambda self: self._pool.fed)
    nll_sum = property(lambda self: self._pool.nll_sum)

    def join(self, conditions=None, n=1, slots=None):
        n = int(n) if slots is None else len(slot_list(slots, self.capacity, "join"))
        c = self._owner._conditions(n, conditions)           # (its refusals come before any device work)
        slots = self._pool.join(n, slots)
        for i, u in enumerate(slots):
            self._cond[u] = None if c is None else c[i:i + 1]
        return slots

    def leave(self, slots):
        self._pool.leave(slots)
        for u in slot_list(slots, self.capacity, "leave"):
            self._cond.pop(u, None)

    def room(self, slot):
        return self._pool.room(int(slot))

    def available(self, slot):
        return self._pool.available(int(slot))

    def bits_per_sample(self, slot):
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        return self._pool.bits_per_sample(int(slot))

    def feed(self, slots, encoding):
        """encoding: one [k, latent_channels] array per slot (one slot: the array itself)."""
        if not self._owner.conditioned:
            raise ValueError("feed: this teacher is not conditioned")
        one = np.isscalar(slots) or (isinstance(encoding, (np.ndarray, torch.Tensor)) and encoding.ndim == 2)
        us = slot_list(slots, self.capacity, "feed")
        pieces = [encoding] if one else list(encoding)
        if len(pieces) != len(us):
            raise ValueError("feed: %d slots but %d pieces of encoding" % (len(us), len(pieces)))
        if any(u not in self._cond for u in us):
            raise ValueError("feed: slots %s do not all hold a stream of this pool" % (us,))
        self._pool.feed(us, [self._owner._frames(torch.as_tensor(e, dtype=torch.float32)[None], self._cond[u])[0]
                             for u, e in zip(us, pieces)])

    def step(self, return_logits=False):
        out = self._pool.step(return_logits)
        return tuple(_host_dict(d) for d in out) if isinstance(out, tuple) else _host_dict(out)


def _flow_variables(name, flows):
    """Reference name -> tensor over the flows of a student (engines or weight sets): flow i lives under
    ``{name}/Flow{i}/Flow{i}`` (model.py:417,468,510)."""
    out = {}
    for i, f in enumerate(flows):
        out.update(f.tf_variables("%s/Flow%d/Flow%d" % (name, i, i)))
    return out


class _FlowFace(object):
    """What ``StudentSynthesizer`` and ``StudentInverter`` share: the student's hyper-parameters, the flows' variables by
    the reference's names, ``load`` and ``from_checkpoint``.  ``_eng`` holds the flows' ``weights``."""

    _repack_each = False      # (the inverter reads each flow's own weight images too)

    def _hyper(self, dilations, num_flows, filter_width, dilation_channels, latent_channels, condition_size, pool_stride,
               name, dtype, **cfg):
        """Keeps the hyper-parameters; returns the flows' ``StackConfig``."""
        self.dilations, self.num_flows = list(dilations), int(num_flows)
        self.filter_width, self.dilation_channels = filter_width, dilation_channels
        self.latent_channels, self.condition_size, self.pool_stride = latent_channels, condition_size, pool_stride
        self._name = name
        return StackConfig(dilations=list(dilations), filter_width=filter_width, dilation_channels=dilation_channels,
                           cond_channels=latent_channels + condition_size, pool_stride=pool_stride,
                           dtype=dtype or _default_dtype(), **cfg)

    @property
    def network_params(self):
        return _flow_variables(self._name, self._eng.weights)

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            if self._repack_each:
                for w in self._eng.weights:
                    w.repack()
            self._eng.repack()
        return ok

    @classmethod
    def from_checkpoint(cls, logdir, dilations, num_flows, **kwargs):
        """This face on the flows saved in `logdir` (``ParallelWaveNet.save``); the hyper-parameters are the
        constructor's (the student's checkpoint holds variables only)."""
        face = cls(dilations, num_flows, **kwargs)
        if not face.load(logdir):
            raise FileNotFoundError("%s: no student checkpoint (ParallelWaveNet.save writes one)" % logdir)
        return face


class StudentSynthesizer(_FlowFace):
    """The deployable form of the student: the flows of a trained ``ParallelWaveNet`` (model.py:415-535) as a streaming
    synthesizer (``student.FlowSynthesizer``), with no teacher anywhere.  It serves any batch <= ``max_batch`` and any
    length = frames * pool_stride with frames <= ``max_frames``, in one call (``synthesize``) or chunk by chunk
    (``stream``), and streams of any length whose encoding arrives while they run (``live``); the noise is drawn on the
    device from per-stream seeds (or given).  ``load`` reads what
    ``ParallelWaveNet.save`` wrote, by the reference's variable names; the gate and skip variables a flow never reads are
    ignored."""

    def __init__(self, dilations, num_flows, filter_width=2, dilation_channels=32, latent_channels=16, condition_size=0,
                 pool_stride=512, name="ParallelWaveNet", dtype=None, max_batch=1, max_chunk=1600, max_frames=32):
        K._need_gpu()
        from .student import FlowSynthesizer
        cfg = self._hyper(dilations, num_flows, filter_width, dilation_channels, latent_channels, condition_size,
                          pool_stride, name, dtype)
        self.max_batch, self.max_chunk, self.max_frames = int(max_batch), int(max_chunk), int(max_frames)
        self._eng = FlowSynthesizer(cfg, num_flows, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)

    # ------------------------------------------------------------------------------------------------
    def _begin(self, encoding, conditions, seed, temperature, noise):
        enc = np.asarray(encoding, dtype=np.float32)
        if enc.ndim != 3 or enc.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels=%d]" % self.latent_channels)
        B, frames = int(enc.shape[0]), int(enc.shape[1])
        if not 1 <= B <= self.max_batch or not 1 <= frames <= self.max_frames:
            raise ValueError("encoding of %d streams x %d frames: this synthesizer was built for max_batch=%d, max_frames=%d"
                             % (B, frames, self.max_batch, self.max_frames))
        e = torch.as_tensor(enc)
        if self.condition_size > 0:
            if conditions is None:
                raise ValueError("this student was built with condition_size > 0; pass conditions [B, condition_size]")
            c = np.asarray(conditions, dtype=np.float32)
            if c.shape != (B, self.condition_size):
                raise ValueError("conditions must be [%d, %d]" % (B, self.condition_size))
            e = _tile_conditions(e, torch.as_tensor(c))
        T = frames * self.pool_stride
        nz = None
        if noise is not None:
            nz = torch.as_tensor(np.asarray(noise, dtype=np.float32))
            if tuple(nz.shape) == (B, T, 1):      # (what StudentInverter.invert returns)
                nz = nz[:, :, 0]
            if tuple(nz.shape) != (B, T):
                raise ValueError("noise must be [%d, %d] (= frames * pool_stride)" % (B, T))
            nz = nz.to("cuda")
        st = self._eng.start(e.contiguous(), seed, temperature)
        return st, nz, B, T

    def _chunks(self, st, nz, T, size):
        t = 0
        while t < T:
            n = min(size, T - t)
            yield self._eng.step(st, n, None if nz is None else nz[:, t:t + n])
            t += n

    def synthesize(self, encoding, conditions=None, seed=0, temperature=1.0, noise=None):
        """encoding [B, frames, latent_channels] -> audio [B, frames * pool_stride, 1] in [-1, 1] (model.py:535), made in
        chunks of max_chunk.  seed / temperature: scalars or one per stream (a scalar seed s: stream b draws with s + b);
        noise [B, T] (or [B, T, 1], as ``StudentInverter.invert`` returns it): the logistic noise itself
        (``ParallelWaveNet.generate``'s `inputs`)."""
        st, nz, B, T = self._begin(encoding, conditions, seed, temperature, noise)
        out = torch.cat(list(self._chunks(st, nz, T, self.max_chunk)), dim=1)
        return out.view(B, T, 1).cpu().numpy()

    def stream(self, encoding, conditions=None, chunk_size=160, seed=0, temperature=1.0, noise=None):
        """The same audio as an iterator of NumPy [B, chunk, 1] blocks (the last one shorter when chunk_size does not
        divide the length); chunking never changes a sample."""
        chunk_size = int(chunk_size)
        if not 1 <= chunk_size <= self.max_chunk:
            raise ValueError("chunk_size %d: 1..max_chunk = %d" % (chunk_size, self.max_chunk))
        st, nz, B, T = self._begin(encoding, conditions, seed, temperature, noise)
        return (c.view(B, -1, 1).cpu().numpy() for c in self._chunks(st, nz, T, chunk_size))

    def pool(self):
        """A ``SynthesisPool`` on this synthesizer's buffers: ``max_batch`` slots that streams join and leave while it
        runs.  It ends a running ``stream``; the next ``synthesize`` / ``stream`` closes the pool."""
        K._need_gpu()
        return SynthesisPool(self._eng.pool(), self.latent_channels, self.condition_size)

    def live(self, batch, conditions=None, seed=0, temperature=1.0):
        """A ``LiveSynthesis`` of `batch` streams whose encoding arrives while they run: ``feed`` frames, ``step`` samples,
        with no bound on the length (the conditioning tables are rings of ``max_frames`` frames).  conditions
        [batch, condition_size] are tiled onto every fed frame.  It ends a running ``stream`` or pool, like ``synthesize``."""
        K._need_gpu()
        return LiveSynthesis(self, int(batch), conditions, seed, temperature)

    def inverter(self, max_batch=None):
        """A ``StudentInverter`` on this synthesizer's own flow weights (one snapshot serves both directions):
        ``synth.synthesize(encoding, conditions, noise=inv.invert(x, encoding, conditions))`` is the round trip."""
        return StudentInverter(self.dilations, self.num_flows, filter_width=self.filter_width,
                               dilation_channels=self.dilation_channels, latent_channels=self.latent_channels,
                               condition_size=self.condition_size, pool_stride=self.pool_stride, name=self._name,
                               dtype=self._eng.dt, max_batch=self.max_batch if max_batch is None else max_batch,
                               _share=self._eng)


class StudentInverter(_FlowFace):
    """The reverse direction of the student (``student.FlowInverter``): audio in, out the logistic noise that the flows of
    a trained ``ParallelWaveNet`` (model.py:456-535) turn into it, and its exact log-likelihood under the student,
    nll[b, t] = -log logistic(z[b, t]; 0, 1) + sum over the flows of their log scales at t (nats).  The inverse of an
    autoregressive flow is sequential: one persistent launch per flow and chunk steps through the samples.

    The audio is taken as the flows' UNCLIPPED output: samples that the student clipped at +-1 (model.py:535) do not
    invert to the noise that made them.  ``load`` reads what ``ParallelWaveNet.save`` wrote."""

    def __init__(self, dilations, num_flows, filter_width=2, dilation_channels=32, latent_channels=16, condition_size=0,
                 pool_stride=512, name="ParallelWaveNet", dtype=None, max_batch=1, gate_mode="reference", _share=None):
        from .student import FlowInverter
        cfg = self._hyper(dilations, num_flows, filter_width, dilation_channels, latent_channels, condition_size,
                          pool_stride, name, dtype, gate_mode=gate_mode)
        self.max_batch = int(max_batch)
        if _share is None:
            self._eng = FlowInverter(cfg, num_flows, max_batch=max_batch)
        else:      # a FlowSynthesizer: its weights
            self._eng = FlowInverter(cfg, num_flows, max_batch=max_batch, device=_share.dev, weights=_share.weights)

    _repack_each = True

    # ------------------------------------------------------------------------------------------------
    def _cond(self, encoding, conditions):
        """encoding [B, frames, latent] (+ conditions [B, condition_size]) -> encoding_w_condition as a host tensor; every
        refusal, no device work."""
        enc = np.asarray(encoding, dtype=np.float32)
        if enc.ndim != 3 or enc.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels=%d]" % self.latent_channels)
        B = int(enc.shape[0])
        if not 1 <= B <= self.max_batch or enc.shape[1] < 1:
            raise ValueError("encoding of %d streams x %d frames: this inverter was built for max_batch=%d"
                             % (B, enc.shape[1], self.max_batch))
        c = _check_conditions(B, conditions, self.condition_size, "student")
        e = torch.as_tensor(enc)
        return e if c is None else _tile_conditions(e, torch.as_tensor(c))

    def _audio(self, audio, batch, length=None):
        x = np.asarray(audio, dtype=np.float32)
        if x.ndim == 3 and x.shape[2] == 1:
            x = x[:, :, 0]
        if x.ndim != 2 or x.shape[0] != batch or (length is not None and x.shape[1] != length):
            raise ValueError("audio must be [%d, %s], got %s" % (batch, "n" if length is None else length, np.shape(audio)))
        return x

    def _invert(self, audio, encoding, conditions):
        from .student import logistic_nll
        e = self._cond(encoding, conditions)
        x = self._audio(audio, e.shape[0], e.shape[1] * self.pool_stride)
        z, ls = self._eng.invert(torch.as_tensor(x), e.contiguous())
        return z, logistic_nll(z, ls)

    def invert(self, audio, encoding, conditions=None):
        """audio [B, T = frames * pool_stride] (or [B, T, 1]) -> noise [B, T, 1], ``ParallelWaveNet.generate``'s `inputs`."""
        z, _ = self._invert(audio, encoding, conditions)
        return z.view(z.shape[0], -1, 1).cpu().numpy()

    def log_likelihood(self, audio, encoding, conditions=None):
        """-log p(audio[b, t] | audio[b, < t], encoding) under the student, [B, T] in nats."""
        return self._invert(audio, encoding, conditions)[1].cpu().numpy()

    def stream(self, encoding, conditions=None):
        """An ``InversionStream`` over the encoding: ``push`` audio chunk by chunk; chunking never changes a bit."""
        e = self._cond(encoding, conditions)
        return InversionStream(self, self._eng.start(e.contiguous()))


class InversionStream(object):
    """NumPy face of one running batch of inversion streams (``StudentInverter.stream``).  ``t``: samples inverted per
    stream."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B
        self._nll_sum = np.zeros(state.B, np.float64)

    @property
    def t(self):
        return self._st.t

    def push(self, audio):
        """audio [B, n] -> (noise [B, n], nll [B, n]) of exactly those samples.  A push past frames * pool_stride is
        refused (ValueError) and leaves the stream where it was."""
        from .student import logistic_nll
        x = self._owner._audio(audio, self._st.B)
        z, ls = self._owner._eng.step(self._st, torch.as_tensor(x))
        nll = logistic_nll(z, ls).cpu().numpy()
        self._nll_sum += nll.sum(1, dtype=np.float64)
        return z.cpu().numpy(), nll

    def bits_per_sample(self):
        """Mean nll of everything pushed so far, in bits, per stream [B] (NaN before the first sample)."""
        from .scorer import bits_per_sample
        return np.array([bits_per_sample(v, self._st.t) for v in self._nll_sum])


class LiveSynthesis(_LiveStream):
    """One running batch of live streams (``StudentSynthesizer.live``).  ``feed(encoding [B, k, latent])`` hands every
    stream its next k frames (k <= ``room``), ``step(n)`` returns the next n <= ``available`` samples [B, n, 1]; ``t``:
    samples made so far.  The samples are those ``synthesize`` gives the whole encoding with the same seed and
    temperature, however the frames and chunks were cut."""

    def __init__(self, owner, batch, conditions, seed, temperature):
        if not 1 <= batch <= owner.max_batch:
            raise ValueError("batch %d: this synthesizer was built for max_batch=%d" % (batch, owner.max_batch))
        cond = _device_conditions(batch, conditions, owner.condition_size, "student")
        super().__init__(owner, owner._eng.start(None, seed, temperature, live=True, batch=batch), cond, batch,
                         owner.max_frames)

    @property
    def room(self):
        return self._owner._eng.room(self._st)

    def _take(self, e):
        self._owner._eng.feed(self._st, e)

    def _step_device(self, n):
        return self._owner._eng.step(self._st, n)

    def step(self, n):
        n = int(n)
        return self._step_device(n).view(self.batch_size, n, 1).cpu().numpy()


class SynthesisPool(_PoolFace):
    """NumPy face of a student synthesis pool (student.SynthPool): ``join(encoding=[...], ...)`` takes one
    [frames_i, latent] per stream and returns their slots; ``step(n)`` advances every live slot by n samples with the
    launches of one synthesizer chunk and returns ``{slot: samples}`` of every slot that produced some; a stream that
    reaches its end frees its slot; ``leave(slots)`` ends streams early.  A stream's samples put together are what
    ``StudentSynthesizer.synthesize`` of that stream alone returns with its seed and temperature."""

    def __init__(self, pool, latent, condition_size):
        self._pool, self._latent, self._cs = pool, latent, condition_size
        self._live_cond = {}      # slot -> the conditions of the live stream joined there last

    t = property(lambda self: self._pool.t)

    def join(self, encoding, conditions=None, seed=0, temperature=None, max_samples=None, live=False):
        """encoding: one [frames_i, latent] per stream (a single 2-D array: one stream); conditions: one [condition_size]
        per stream, tiled over its frames; seed: one per stream or a scalar s (stream i draws with s + i).
        live=True: the streams are fed while they run (``feed``); an encoding holds a stream's first frames ([0, latent]:
        none yet), its conditions are kept and tiled onto every frame fed later; a live stream that has used up its frames
        waits (no samples) until it is fed, closed or left."""
        if live:
            K._need_gpu()
        if isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
            conditions = None if conditions is None else [conditions]
        encoding = list(encoding)
        cond = _pool_encodings(len(encoding), encoding, conditions, self._latent, self._cs)
        slots = self._pool.join(cond, seed, temperature, max_samples, live=live)
        if live and self._cs > 0:
            for u, c in zip(slots, per_stream(conditions, len(slots), "conditions")):
                self._live_cond[u] = np.asarray(c, dtype=np.float32).reshape(1, self._cs)
        return slots

    def feed(self, slots, encoding):
        """The next frames of live slots: encoding[i] [k_i, latent] for slots[i] (k_i <= ``room``)."""
        slots = slot_list(slots, self.capacity, "feed")
        if isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
        encs = [np.asarray(e, dtype=np.float32) for e in encoding]
        if len(encs) != len(slots):
            raise ValueError("feed: %d slots but %d encodings" % (len(slots), len(encs)))
        for e in encs:
            if e.ndim != 2 or e.shape[1] != self._latent:
                raise ValueError("feed: each encoding is [k, %d], got shape %s" % (self._latent, e.shape))
        if self._cs > 0:
            if any(u not in self._live_cond for u in slots):
                raise ValueError("feed: slots %s are not all live streams of this pool" % (slots,))
            encs = [_tile_conditions_np(e, self._live_cond[u]) for u, e in zip(slots, encs)]
        self._pool.feed(slots, encs)

    def room(self, slot):
        return self._pool.room(int(slot))

    def close(self, slots):
        """No more frames will come for these live streams: each frees its slot at the end of what it was fed."""
        self._pool.close(slots)

    def step(self, n):
        a, ran = self._pool.step(int(n))
        return _ran_dict(a, ran, range(self._pool.capacity))


class Resynthesizer(object):
    """The live pipeline: an ``AudioEncoder`` feeding a ``StudentSynthesizer``.  Audio chunks in, resynthesized audio
    chunks out, with no bound on the length; the latent frames go from the encoder into the synthesizer's conditioning
    rings as device tensors and never visit the host.  Both halves keep their own contracts, so the audio of a stream put
    together equals ``synthesizer.synthesize(encoder.encode(audio), ...)`` however the audio was cut."""

    def __init__(self, encoder, synthesizer):
        K._need_gpu()
        self.lookahead = _check_resynthesis_halves("Resynthesizer", encoder, synthesizer, StudentSynthesizer, "synthesizer",
                                                   "synthesizer")
        cs = synthesizer.condition_size
        if synthesizer._eng.E != encoder.latent_channels + cs:
            raise ValueError("condition_size %d: the synthesizer's flows read %d channels, not %d + %d"
                             % (cs, synthesizer._eng.E, encoder.latent_channels, cs))
        self.encoder, self.synthesizer = encoder, synthesizer
        self.pool_stride = int(encoder.pool_stride)

    def stream(self, batch=1, conditions=None, seed=0, temperature=1.0, chunk_size=160):
        """A ``ResynthesisStream`` of `batch` streams in lockstep: ``push(audio [B, m])`` returns every sample that can be
        made by now, [B, m', 1]; ``finish()`` the rest.  conditions [B, condition_size] are tiled onto every frame on the
        device (model.py:496-499); chunk_size: the largest synthesizer chunk."""
        batch, chunk_size = int(batch), int(chunk_size)
        if not 1 <= batch <= min(self.encoder.max_batch, self.synthesizer.max_batch):
            raise ValueError("batch %d: the encoder holds %d streams, the synthesizer %d"
                             % (batch, self.encoder.max_batch, self.synthesizer.max_batch))
        if not 1 <= chunk_size <= self.synthesizer.max_chunk:
            raise ValueError("chunk_size %d: 1..max_chunk = %d" % (chunk_size, self.synthesizer.max_chunk))
        return ResynthesisStream(self, batch, conditions, seed, temperature, chunk_size)

    def pool(self, chunk_size=160, audio_ring=None):
        """A ``ResynthesisPool``: independent callers on one encoder and one synthesizer.  Streams join and leave while the
        batch runs, audio arrives ragged, and each caller receives what it would have received alone.  chunk_size: the
        samples a ``step`` makes per stream at most; audio_ring: samples of audio a slot can hold (``AudioEncoder.pool``)."""
        K._need_gpu()
        return ResynthesisPool(self, int(chunk_size), audio_ring)


class ResynthesisStream(_ResynthesisStream):
    """One running batch of ``Resynthesizer.stream``: ``push`` / ``finish`` return samples [B, m, 1]."""

    _tail = (1,)

    def _start_live(self, batch, conditions, seed, temperature):
        return self._owner.synthesizer.live(batch, conditions, seed, temperature)


class _ResynthesisPool(SlotTable):
    """What ``ResynthesisPool`` and ``TeacherResynthesisPool`` share: an encoder pool ``_enc`` and a live decoding half
    ``_half`` (a pool with ``room`` / ``feed`` / ``close`` / ``leave`` / ``t`` and ``_active``) sharing slot ids, the
    streams' conditions ``_cond`` (slot -> [1, condition_size] on the device, None without: a slot is taken while it has an
    entry), ``_cs`` and ``_chunk``.  A subclass gives ``_half``, ``_half_join`` and ``_half_step``.
    One ``step``: the encoder emits for each slot at most the frames the decoding half's conditioning ring has room for
    (the rest stays audio in the slot's audio ring: there is no second queue), the new frames are fed as device tensors
    with the slot's conditions tiled on, the slots whose audio is finished and fully encoded are closed, and the
    decoding half makes up to ``chunk_size`` samples per slot.  A stream that reaches its end frees its slot in both
    halves."""

    _who = "student"

    @property
    def _active(self):      # (what SlotTable reads: a slot is taken while it has an entry in _cond)
        return np.array([u in self._cond for u in range(self.capacity)], bool)

    @property
    def t(self):
        """Samples returned so far, per slot."""
        return self._half.t[:self.capacity]

    @property
    def received(self):
        return self._enc.received[:self.capacity]

    def audio_room(self, slot):
        return self._enc.audio_room(int(slot))

    def _slots(self, slots, who):
        slots = self._slot_list(slots, who)
        if any(u not in self._cond for u in slots):
            raise ValueError("%s: slots %s do not all hold a stream of this pool" % (who, slots))
        return slots

    def join(self, conditions=None, seed=0, temperature=None, n=1):
        """n streams into the lowest free slots; conditions [n, condition_size] (one row per stream), seed a scalar s
        (stream i draws with s + i) or one per stream, temperature None, a scalar or one per stream.  Returns the slots."""
        n = int(n)
        slots = self._take_slots(n, None)
        c = _device_conditions(n, conditions, self._cs, self._who)
        conds = [None if c is None else c[i:i + 1] for i in range(n)]
        self._half_join(n, seed, temperature, slots)
        self._enc.join(slots=slots)
        for u, c in zip(slots, conds):
            self._cond[u] = c
        return slots

    def push(self, slots, audio):
        self._enc.push(self._slots(slots, "push"), _audio_pieces(slots, audio))

    def finish(self, slots):
        """No more audio comes for these streams; each frees its slot once its last sample has been returned."""
        self._enc.finish(self._slots(slots, "finish"))

    def leave(self, slots):
        """Ends these streams where they are and frees their slots in both halves."""
        slots = self._slots(slots, "leave")
        self._enc.leave(slots)
        self._half.leave(slots)
        for u in slots:
            del self._cond[u]

    def step(self):
        if not self._cond:
            return {}
        enc, half = self._enc, self._half
        frames = enc.step({u: half.room(u) for u in enc.active})
        if frames:
            us = sorted(frames)
            fr = [frames[u] if self._cond[u] is None else _tile_conditions(frames[u][None], self._cond[u])[0] for u in us]
            half.feed(us, fr)
        done = [u for u in self._cond if not enc._active[u]]          # finished and fully encoded: the stream's end is known
        if done:
            half.close(done)
        a, ran = self._half_step(self._chunk)
        out = _ran_dict(a, ran, self._cond) if ran.any() else {}
        for u in [u for u in self._cond if not half._active[u]]:
            del self._cond[u]
        return out


class ResynthesisPool(_ResynthesisPool):
    """``Resynthesizer.pool()``: an encoder pool and a live synthesis pool sharing slot ids; capacity is the smaller
    ``max_batch``.  ``join`` returns slots, ``push(slots, audio)`` takes one 1-D array per slot of any length (at most
    ``audio_room(slot)``), ``finish(slots)`` ends streams, ``step()`` returns ``{slot: samples}`` (``_ResynthesisPool``:
    frames the synthesizer's ring has room for, fed as device tensors; up to ``chunk_size`` samples per slot).  A stream's
    samples put together are ``synthesizer.synthesize(encoder.encode(audio), conditions, seed, temperature)`` of it
    alone."""

    def __init__(self, owner, chunk_size, audio_ring):
        from .student import live_min_frames
        enc, syn = owner.encoder, owner.synthesizer
        if not 1 <= chunk_size <= syn.max_chunk:
            raise ValueError("chunk_size %d: 1..max_chunk = %d" % (chunk_size, syn.max_chunk))
        need = live_min_frames(max(syn._eng.hist), owner.pool_stride)
        if syn.max_frames < need:
            raise ValueError("pool: live streams need a synthesizer ring of max_frames >= %d frames, this one holds %d"
                             % (need, syn.max_frames))
        self._owner, self._chunk = owner, chunk_size
        self.capacity = min(enc.max_batch, syn.max_batch)
        self._cs = syn.condition_size
        self._enc = enc._eng.pool(audio_ring)
        self._syn = syn._eng.pool()
        self._cond = {}        # slot -> its stream's conditions [1, condition_size] on the device (None without)

    _half = property(lambda self: self._syn)

    def _half_join(self, n, seed, temperature, slots):
        self._syn.join([None] * n, seed, temperature, slots=slots, live=True)

    def _half_step(self, chunk):
        return self._syn.step(chunk)


class TeacherResynthesisPool(_ResynthesisPool):
    """``TeacherResynthesizer.pool()``: an encoder pool and a LIVE generation pool of the decoder sharing slot ids;
    capacity is the encoder's ``max_batch``, the decoder's conditioning rings hold ``max_frames`` frames.  The contract of
    ``ResynthesisPool`` at teacher quality: ``join`` returns slots, ``push(slots, audio)`` takes one 1-D array per slot of
    any length (at most ``audio_room(slot)``), ``finish(slots)`` ends streams, ``step()`` returns ``{slot: samples}``.  A
    stream's samples put together are ``autoencoder.generate(encoder.encode(audio), conditions, seed=seed,
    temperature=temperature)`` of it alone."""

    _who = "auto-encoder"

    def __init__(self, owner, chunk_size, audio_ring):
        if chunk_size < 1:
            raise ValueError("chunk_size %d: at least 1" % chunk_size)
        enc, ae = owner.encoder, owner.autoencoder
        self._owner, self._chunk = owner, chunk_size
        self.capacity = int(enc.max_batch)
        self._cs = int(ae.condition_size)
        self._enc = enc._eng.pool(audio_ring)
        eng = ae._eng or ae._engine(1, owner.max_frames * owner.pool_stride)
        self._dec = eng.dec.generation_pool(self.capacity, owner.max_frames, live=True)
        self._cond = {}        # slot -> its stream's conditions [1, condition_size] on the device (None without)

    _half = property(lambda self: self._dec)

    def _half_join(self, n, seed, temperature, slots):
        sd = np.asarray(seed)
        seeds = [int(sd) + i for i in range(n)] if sd.ndim == 0 else [int(v) for v in per_stream(seed, n, "seeds", default=0)]
        self._dec.join(seeds, None, [None] * n, None, slots, temperature=temperature, live=True)

    def _half_step(self, chunk):
        dec = self._dec
        if not dec.any_runnable:      # every stream waits for frames: nothing is launched
            return None, np.zeros(self.capacity, np.int64)
        a, _, _, ran = dec.step(chunk, mode="sample")
        return a, ran


def _embed_host(r, threshold=None):
    """An ``embedder.EmbedResult`` of device tensors -> one of NumPy arrays; with a threshold (result, accepted)."""
    out = type(r)(*(t.cpu().numpy() for t in r))
    return out if threshold is None else (out, out.distance <= np.float32(threshold))


class StreamingEmbedder(object):
    """The deployable form of a ``SiameseWaveNet`` tower (model.py:689-731) with a NumPy face: no training engine, no clip
    length, and a gallery of enrolled templates on the device.  ``embed(audio [B, T])`` -> an ``EmbedResult`` (embeddings
    [B, n_emit, D], nearest [B, n_emit], distance [B, n_emit], distances [B, n_emit, N]) of every window position (j + 1) *
    hop - window, j >= window / hop - 1, of a recording of any length: the reference's distance (model.py:736) to each of
    the N enrolled templates, the nearest one's index (-1 with none enrolled) and its distance.  ``enroll(clips [n,
    window])`` embeds clips with this object's own path and adds them; ``stream(batch)`` -> an ``EmbedderStream`` to
    ``push`` audio into as it arrives.  A result does not depend on how the audio was cut."""

    def __init__(self, weights, max_batch=1, hop=160, window=16000, max_hops=8, max_gallery=64):
        from .embedder import StreamEmbedder
        self._w = weights
        self._eng = StreamEmbedder(weights, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops,
                                   max_gallery=max_gallery)
        e = self._eng
        self.max_batch, self.hop, self.window, self.max_gallery, self.output_dimensions = (e.max_batch, e.hop, e.window,
                                                                                           e.max_gallery, e.D)

    @classmethod
    def from_checkpoint(cls, logdir, dilations, output_dimensions, dilation_channels=32, skip_channels=256, filter_width=2,
                        name="SiameseWaveNet", dtype=None, max_batch=1, hop=160, window=16000, max_hops=8, max_gallery=64):
        """An embedder on the variables saved in `logdir` (``SiameseWaveNet.save``'s .pt form or a TensorFlow bundle, by the
        reference's variable names under `name`/siamese)."""
        from .embedder import EmbedderWeights, check_gallery_size
        from .recognizer import check_classifier_widths, check_hop_window
        check_hop_window(hop, window)
        check_gallery_size(max_gallery)
        check_classifier_widths(filter_width, dilation_channels, skip_channels, "streaming embedder")
        w = EmbedderWeights(dilations, dilation_channels, skip_channels, output_dimensions, filter_width,
                            dtype or _default_dtype())
        if not w.load(logdir, name + "/siamese"):
            raise FileNotFoundError("%s: no checkpoint to restore (SiameseWaveNet.save writes one)" % logdir)
        return cls(w, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops, max_gallery=max_gallery)

    gallery = property(lambda self: self._eng.gallery.cpu().numpy(), doc="The enrolled templates [N, D].")
    labels = property(lambda self: self._eng.labels, doc="One label per enrolled template.")

    def embed(self, inputs):
        """inputs [B, T] -> ``EmbedResult`` (NumPy) of the n_emit = max(0, T // hop - window / hop + 1) window positions."""
        return _embed_host(self._eng.embed(self._eng._check_audio(inputs)))

    def enroll(self, inputs, labels=None):
        """Embeds the clips inputs [n, window] (any n, in batches of max_batch) with this object's own path and enrolls
        the single window of each -> their gallery indices.  Ends the current stream or pool."""
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.window:
            raise ValueError("enroll: inputs must be [n, window = %d], got shape %s" % (self.window, x.shape))
        labels = None if labels is None else list(labels)
        if labels is not None and len(labels) != x.shape[0]:
            raise ValueError("enroll: %d clips but %d labels" % (x.shape[0], len(labels)))
        if len(self._eng.labels) + x.shape[0] > self.max_gallery:
            raise ValueError("enroll: %d clips behind the %d enrolled, max_gallery is %d"
                             % (x.shape[0], len(self._eng.labels), self.max_gallery))
        if not x.shape[0]:
            return []
        e = torch.cat([self._eng.embed(x[i:i + self.max_batch]).embeddings[:, 0]
                       for i in range(0, x.shape[0], self.max_batch)], 0)
        return self._eng.enroll(e, labels)

    def enroll_embeddings(self, templates, labels=None):
        """Enrolls templates [n, D] that are embeddings already -> their gallery indices."""
        return self._eng.enroll(np.asarray(templates, dtype=np.float32), labels)

    def clear(self):
        self._eng.clear()

    def stream(self, batch_size=1):
        return EmbedderStream(self, self._eng.start(batch_size))

    def pool(self, audio_ring=None):
        """An ``EmbedderStreamPool``: this embedder's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio of any length at a clock of its own, all matched against this embedder's gallery (``embedder.EmbedderPool``).
        Ends the current ``EmbedderStream``; ``stream``, ``embed`` and ``enroll`` end the pool."""
        return EmbedderStreamPool(self._eng.pool(audio_ring))


class EmbedderStream(object):
    """NumPy face of one running batch of embedder streams (``StreamingEmbedder.stream``).  ``t``: samples received per
    stream; ``emitted``: window positions returned so far."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B

    t = property(lambda self: self._st.t)
    emitted = property(lambda self: self._st.emitted)

    def push(self, audio, threshold=None):
        """audio [B, n], any n >= 0 -> the ``EmbedResult`` [B, e, ..] of the e window positions it completed (e may be 0);
        with a threshold (result, accepted [B, e] = distance <= threshold)."""
        return _embed_host(self._owner._eng.push(self._st, audio), threshold)


class EmbedderStreamPool(_AudioPoolFace):
    """NumPy face of an embedder pool (``StreamingEmbedder.pool``; embedder.EmbedderPool).  ``join`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``step()`` returns ``{slot: EmbedResult [e, ..]}`` for
    every slot whose stream completed window positions.  A stream's results put together are ``StreamingEmbedder.embed`` of
    its audio alone under the same gallery."""

    audio_ring = property(lambda self: self._pool.audio_ring)
    consumed = property(lambda self: self._pool.consumed)

    def step(self, threshold=None):
        return {u: _embed_host(r, threshold) for u, r in self._pool.step().items()}


class AutoEncoderScorerPool(_ResynthesisPool):
    """``AutoEncoderScorer.pool()``: an encoder pool ``_enc`` and a ``scorer.MolScorerPool`` ``_mol`` sharing slot ids, with
    the contract of the resynthesis pools; capacity is the smaller ``max_batch``.  ``join(conditions, n)`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot of any length (at most ``audio_room(slot)``) and writes it into BOTH
    halves' audio rings (two uploads: the halves keep separate rings), ``finish(slots)`` ends streams, ``leave(slots)``
    drops them, ``step()`` returns ``{slot: nll [m]}`` (NumPy, nats).  One ``step``: the encoder emits for each slot at most
    the frames the scorer's conditioning ring has room for (the rest stays audio), the new frames are fed as device
    tensors with the slot's conditions tiled on, the scorer scores every sample that has its frame, and a slot whose
    encoder half is finished and fully emitted and whose scorer half has scored all it was fed is freed in both halves.
    A stream's values put together are ``AutoEncoderScorer(max_batch=1).score(audio)`` of it alone: its first (T //
    pool_stride) * pool_stride samples; a stream shorter than one frame ends with nothing.
    The scorer half's audio ring must hold what the ENCODER still needs before it can emit the next frame -- with every
    fed sample scored that is pool_stride + L + 1 samples beyond emitted * pool_stride, plus the two samples the entry
    conv carries -- or neither half could move: ``scorer.ae_pool_min_audio_ring``, refused below."""

    _who = "scorer"

    def __init__(self, owner, audio_ring):
        from .scorer import ae_pool_min_audio_ring
        enc, mol = owner.encoder._eng, owner._eng
        need = ae_pool_min_audio_ring(mol.max_chunk, enc.P, enc.L)
        enc_ring = enc.max_frames * enc.P + enc.L + 1 + enc.P            # (the encoder pool's default)
        ring = enc_ring + mol.max_chunk + 2 if audio_ring is None else int(audio_ring)
        if ring < need:
            raise ValueError("pool: audio_ring %d: the scorer half needs at least %d samples (a step of max_chunk + 2 = %d, "
                             "and pool_stride + encoder layers + 3 = %d so that the encoder can complete its next frame)"
                             % (ring, need, mol.max_chunk + 2, enc.P + enc.L + 3))
        self._owner = owner
        self.capacity = min(enc.max_batch, mol.max_batch)
        self._cs = owner.condition_size
        self._enc = enc.pool()
        self._mol = mol.pool(ring)
        self._cond = {}        # slot -> its stream's conditions [1, condition_size] on the device (None without)

    _half = property(lambda self: self._mol)
    t = property(lambda self: self._mol.scored[:self.capacity], doc="Samples scored so far, per slot.")
    scored = t

    def audio_room(self, slot):
        """Samples a slot can take now: the smaller of the two halves' rooms."""
        return min(self._enc.audio_room(int(slot)), self._mol.audio_room(int(slot)))

    def bits_per_sample(self, slot):
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        return self._mol.bits_per_sample(int(slot))

    def join(self, conditions=None, n=1):
        """n streams into the lowest free slots; conditions [n, condition_size] (one row per stream).  Returns the slots."""
        n = int(n)
        self._mol._check_open()
        slots = self._take_slots(n, None)
        c = _device_conditions(n, conditions, self._cs, self._who)
        self._mol.join(slots=slots)
        self._enc.join(slots=slots)
        for i, u in enumerate(slots):
            self._cond[u] = None if c is None else c[i:i + 1]
        return slots

    def push(self, slots, audio):
        """Each piece into both halves' rings.  A piece that fits one half only is refused before either is written, as
        is everything either half refuses."""
        pieces = _audio_pieces(slots, audio)
        slots = self._slots(slots, "push")
        self._mol._check_open()
        if len(pieces) != len(slots):
            raise ValueError("push: %d slots but %d pieces of audio" % (len(slots), len(pieces)))
        for u, x in zip(slots, pieces):
            if x.ndim == 1 and x.shape[0] > self.audio_room(u):
                raise ValueError("push: %d samples for slot %d, but its rings have room for %d (encoder half %d, scorer half "
                                 "%d)" % (x.shape[0], u, self.audio_room(u), self._enc.audio_room(u), self._mol.audio_room(u)))
        self._enc.push(slots, pieces)      # (its refusals -- a finished stream, a wrong dtype or rank -- come before it writes)
        self._mol.push(slots, pieces)

    def leave(self, slots):
        """Ends these streams where they are and frees their slots in both halves."""
        self._mol._check_open()
        super().leave(slots)

    def step(self):
        self._mol._check_open()
        if not self._cond:
            return {}
        enc, mol, P = self._enc, self._mol, self._owner.pool_stride
        frames = enc.step({u: mol.room(u) for u in enc.active})      # frames that do not fit stay audio
        if frames:
            us = sorted(frames)
            mol.feed(us, [frames[u] if self._cond[u] is None else _tile_conditions(frames[u][None], self._cond[u])[0]
                          for u in us])
        out = mol.step()
        done = [u for u in self._cond if not enc._active[u] and mol._scored[u] == mol._fed[u] * P]
        if done:                                                     # finished, fully encoded and fully scored
            mol.leave(done)
            for u in done:
                del self._cond[u]
        return _host_dict(out)
