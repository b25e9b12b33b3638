"""A tower of class ``SiameseWaveNet`` (model.py:660-797) as a standalone streaming embedder with gallery matching: audio
of any length in, the embedding of a sliding window and its distance to every enrolled template out.

A Siamese tower is class ``WaveNet``'s network up to the last 1x1 and the average pool (model.py:689-731), so everything up
to the hop sums is the streaming classifier's (``recognizer.StreamClassifier``: the entry, the stack with stored z,
``srwn_pooled_stream_head`` into the ring of hop sums, the roll).  What differs is what a step makes of the ring:

  m_j     = (H_{j-nW+1} + ... + H_j) / window                 the window mean (the pool commutes with the last 1x1)
  e_j     = m_j @ W2 + b2                                     the embedding [D]: the classifier's pooled logits, bit for bit
  d_j[n]  = sqrt(1e-8 + |e_j - g_n|^2),  n < N                the reference's distance (model.py:736) to every enrolled row
  nearest = argmin_n d_j[n] (lowest index on ties), with its distance; -1 and +inf for an empty gallery

in ONE launch, ``srwn_window_embed_match`` (csrc/srwn_embed.hip), so a step is 4 + G launches for G layer groups: entry, G
groups, head, embed-and-match, roll.  ``SRWN_EMBED_FUSED=0`` runs the parity twin instead -- ``srwn_window_mean`` with
logits, then ``srwn_gallery_match`` -- one launch more, the same bits.  ``SRWN_RECOG_FUSED`` keeps its meaning for the hop
sums.  The gallery [max_gallery, D] and its row count live on the device and the kernel reads the count when it runs:
``enroll`` between two pushes needs no new hipGraph.

``StreamEmbedder.pool()`` turns the rows into slots (``EmbedderPool`` on ``ClassifierPool``'s table and audio ring): the
same launch list in its slot forms, one gallery shared by all slots.
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple

import numpy as np
import torch

from . import kernels as K
from ._lib import call
from .engine import WaveNetEngine
from .recognizer import ClassifierPool, RecogState, StackWeights, StreamClassifier, emissions_due
from .stream_stack import nbytes

# What SRWN_EMBED_FUSED means when it is not set: "1" the one-launch head, "0" the parity twin.
EMBED_FUSED_DEFAULT = "1"
MAX_GALLERY = 1024      # srwn.h


class EmbedResult(NamedTuple):
    """What the e window positions of a push gave: ``embeddings`` [.., e, D], ``nearest`` [.., e] (int32 gallery index, -1
    with an empty gallery), ``distance`` [.., e] to that row (+inf with an empty gallery) and ``distances`` [.., e, N] to
    each of the N rows enrolled when the step ran."""
    embeddings: torch.Tensor
    nearest: torch.Tensor
    distance: torch.Tensor
    distances: torch.Tensor


def check_gallery_size(max_gallery):
    if not 1 <= int(max_gallery) <= MAX_GALLERY:
        raise ValueError("max_gallery %r: 1 .. %d" % (max_gallery, MAX_GALLERY))


class EmbedderWeights(StackWeights):
    """The parameters and forward MFMA images of a ``SiameseWaveNet`` tower without the training engine around it
    (``output_channels`` = the embedding's dimensions D).  Built from a ``SiameseWaveNet``'s engine (``from_engine``: a copy
    of its parameters) or filled from a checkpoint directory by the names ``SiameseWaveNet.save`` writes (``load``)."""

    _who = "streaming embedder"

    @classmethod
    def from_engine(cls, eng: WaveNetEngine) -> "EmbedderWeights":
        """A copy of a contrastive-head engine's parameters (``SiameseWaveNet._engine``); later training does not reach it."""
        cfg = eng.cfg
        if cfg.head_mode != "contrastive":
            raise ValueError("a streaming embedder needs the tower of class SiameseWaveNet (head_mode 'contrastive'), "
                             "this engine has %r" % (cfg.head_mode,))
        if cfg.gate_mode != "reference":
            raise NotImplementedError("gate_mode %r is not built for the streaming embedder" % (cfg.gate_mode,))
        if cfg.shift_input or cfg.cond_channels:
            raise ValueError("the classifier's stack has no RightShift and no conditioning (model.py:33-62)")
        return cls(cfg.dilations, cfg.dilation_channels, cfg.skip_channels, cfg.output_channels, cfg.filter_width, cfg.dtype,
                   eng.dev)._copy_engine(eng)

    def load(self, logdir, scope: str = "SiameseWaveNet/siamese") -> bool:
        """``StackWeights.load`` under the left tower's scope (model.py:689), as ``SiameseWaveNet.save`` names it."""
        return super().load(logdir, scope)


class StreamEmbedder(StreamClassifier):
    """``start`` a batch of streams, then ``push`` audio of any length: an ``EmbedResult`` for the window positions that
    audio completed; ``embed`` for whole recordings.  ``enroll`` appends templates to the gallery every push is matched
    against.  A step of h hops is one hipGraph per (batch, h), as the classifier's."""

    _noun = "embedder"

    def __init__(self, weights: EmbedderWeights, max_batch: int = 1, hop: int = 160, window: int = 16000, max_hops: int = 8,
                 max_gallery: int = 64):
        check_gallery_size(max_gallery)
        self.max_gallery = int(max_gallery)
        self.embed_fused = os.environ.get("SRWN_EMBED_FUSED", EMBED_FUSED_DEFAULT) != "0"
        super().__init__(weights, max_batch, hop, window, max_hops)
        self.D = self.w.C
        self.gallery_buf = self._zeros(self.max_gallery, self.D, dt=torch.float32)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.dev)      # the gallery's rows, where the kernel reads them
        self._n = 0
        self._labels: List[object] = []

    def _alloc_emissions(self):
        w, rows, z = self.w, self.max_batch * self.max_hops, self._zeros
        self.emb = z(rows, w.C, dt=torch.float32)
        self.dist = z(rows, self.max_gallery, dt=torch.float32)
        self.nearest = torch.full((rows,), -1, dtype=torch.int32, device=self.dev)
        self.dmin = z(rows, dt=torch.float32)
        self.mean = None if self.embed_fused else z(rows, w.S, dt=torch.float32)      # (the twin's window means)
        self.launches_per_step = 2 + len(self.groups) + (1 if self.fused else 3) + (1 if self.embed_fused else 2)

    def buffer_bytes(self) -> Dict[str, int]:
        """Device bytes by buffer family (DESIGN's table)."""
        out = dict(self.stack.nbytes(), ring=nbytes([self.ring]), audio=nbytes([self.xbuf, self.carry]),
                   emissions=nbytes([self.emb, self.dist, self.nearest, self.dmin, self.mean]),
                   gallery=nbytes([self.gallery_buf, self.count]), images=nbytes([self.w.packed]))
        if not self.fused:
            out["twin r0/r1"] = nbytes([self.r0, self.r1])
        return out

    # ---- the gallery
    @property
    def gallery(self) -> torch.Tensor:
        """The enrolled templates [N, D] fp32 (a copy)."""
        return self.gallery_buf[:self._n].clone()

    @property
    def labels(self) -> list:
        """One label per enrolled template (its index where none was given)."""
        return list(self._labels)

    def enroll(self, templates, labels=None) -> List[int]:
        """Appends templates [n, D] (or one [D]) to the gallery -> their indices.  Refuses (ValueError, nothing changed) a
        wrong shape, labels of another length and more than ``max_gallery`` rows in all."""
        t = templates if isinstance(templates, torch.Tensor) else torch.as_tensor(np.array(templates, dtype=np.float32))
        if t.dim() == 1:
            t = t[None]
        if t.dim() != 2 or t.shape[1] != self.D:
            raise ValueError("enroll: templates must be [n, %d], got shape %s" % (self.D, tuple(t.shape)))
        n = int(t.shape[0])
        labels = None if labels is None else list(labels)
        if labels is not None and len(labels) != n:
            raise ValueError("enroll: %d templates but %d labels" % (n, len(labels)))
        if self._n + n > self.max_gallery:
            raise ValueError("enroll: %d templates behind the %d enrolled, max_gallery is %d" % (n, self._n, self.max_gallery))
        idx = list(range(self._n, self._n + n))
        if n:
            self.gallery_buf[self._n:self._n + n].copy_(t.to(device=self.dev, dtype=torch.float32))
            self._n += n
            self.count.fill_(self._n)
            self._labels += idx if labels is None else labels
        return idx

    def clear(self) -> None:
        """Empties the gallery."""
        self._n, self._labels = 0, []
        self.count.zero_()

    # ---- the step
    def _launch_emit(self, B: int, h: int, when: int, sfx: str):
        """What a step makes of the hop sums: embeddings, distances and the nearest row -- one launch, or the twin's two."""
        w, st = self.w, K._stream()
        w2, b2 = w.view("head_w2").data_ptr(), w.view("head_b2").data_ptr()
        gal = (self.gallery_buf.data_ptr(), self.count.data_ptr(), self.max_gallery)
        out = (self.dist.data_ptr(), self.nearest.data_ptr(), self.dmin.data_ptr(), st)
        if self.embed_fused:
            call("srwn_window_embed_match" + sfx, self.ring.data_ptr(), self.ring_rows, when, B, h, self.hop, self.window, w.S,
                 w2, b2, w.C, w.Cp, *gal, self.emb.data_ptr(), *out)
        else:
            call("srwn_window_mean" + sfx, self.ring.data_ptr(), self.ring_rows, self.mean.data_ptr(), when, B, h, self.hop,
                 self.window, w.S, w2, b2, self.emb.data_ptr(), w.C, w.Cp, st)
            call("srwn_gallery_match", self.emb.data_ptr(), B * h, w.C, *gal, *out)

    def _rows(self, B: int, h: int):
        """Views [B, h, ..] of the step's rows of the four output buffers."""
        r = B * h
        return (self.emb[:r].view(B, h, self.D), self.nearest[:r].view(B, h), self.dmin[:r].view(B, h),
                self.dist[:r].view(B, h, self.max_gallery))

    def _new_pool(self, audio_ring):
        """``pool()`` returns an ``EmbedderPool``: this embedder's ``max_batch`` rows as slots, each a stream at a clock of its
        own, all matched against this embedder's gallery."""
        return EmbedderPool(self, audio_ring)

    def push(self, state: RecogState, audio) -> EmbedResult:
        """The next samples of every stream, audio [B, n] with any n >= 0 -> the ``EmbedResult`` [B, e, ..] of the e window
        positions they completed (e may be 0), matched against the gallery as it is now.  A device tensor is taken as it
        is.  Refuses (ValueError, state untouched) a wrong rank or batch."""
        self._check_state(state)
        x = self._check_audio(audio, state.B).to(device=self.dev, dtype=torch.float32)
        B, N = state.B, self._n
        x = torch.cat([state._rem, x], 1) if state._rem.shape[1] else x
        hops = int(x.shape[1]) // self.hop
        done = state.t - state._rem.shape[1]                  # samples the stack has consumed (hop-aligned)
        first, count = emissions_due(done, done + hops * self.hop, self.hop, self.window)
        new = lambda *s, dt=torch.float32: torch.empty((B, count) + s, dtype=dt, device=self.dev)
        out = EmbedResult(new(self.D), new(dt=torch.int32), new(), new(N))
        at, j = 0, done // self.hop
        for h0 in range(0, hops, self.max_hops):
            h = min(self.max_hops, hops - h0)
            n = h * self.hop
            self.xbuf[:B, :n].copy_(x[:, h0 * self.hop:h0 * self.hop + n])
            K.run_cached_graph(self._graphs, self._seen, (B, h), self.use_graphs, lambda: self._launch_step(B, h))
            skip = min(max(first - j, 0), h)                  # hops of this step before the first full window
            if h > skip:
                emb, near, dmin, dist = self._rows(B, h)
                sl = slice(at, at + h - skip)
                out.embeddings[:, sl] = emb[:, skip:]
                out.nearest[:, sl] = near[:, skip:]
                out.distance[:, sl] = dmin[:, skip:]
                out.distances[:, sl] = dist[:, skip:, :N]
                at += h - skip
            j += h
        state._rem = x[:, hops * self.hop:].clone()
        state.t = done + int(x.shape[1])
        state.emitted += count
        return out

    def embed(self, audio) -> EmbedResult:
        """Whole recordings audio [B, T] of any T -> the ``EmbedResult`` of its n_emit = max(0, T // hop - window / hop + 1)
        window positions; a trailing part that does not fill a hop is not heard.  Starts a new state."""
        x = self._check_audio(audio)
        return self.push(self.start(int(x.shape[0])), x)

    # (the classifier's faces make no sense on a tower)
    def classify(self, audio, return_logits: bool = False):
        raise TypeError("a StreamEmbedder embeds: use embed()")


class EmbedderPool(ClassifierPool):
    """``StreamEmbedder.pool()``: ``ClassifierPool``'s slots, audio ring, ``join`` / ``leave`` / ``push`` / ``audio_room`` and
    pass loop on the embedder's launch list in its slot forms; ``step`` returns ``{slot: EmbedResult}`` with [e, ..] rows.
    One gallery, the owner's, for all slots.  A stream's results put together equal ``StreamEmbedder(max_batch=1).embed`` of
    its audio alone under the same gallery, bit for bit."""

    def step(self) -> Dict[int, EmbedResult]:
        """Runs while any active slot has a whole hop waiting -> {slot: EmbedResult [e, ..] on the device} for the slots
        whose streams completed e > 0 window positions, matched against the gallery as it is now.  With nothing due nothing
        is launched."""
        parts: Dict[int, list] = {}
        for k, due in self._passes():
            if due:      # one copy per pass: the next pass writes the same buffers
                N = self.c._n
                emb, near, dmin, dist = (t.clone() for t in self.c._rows(self.capacity, k))
            for u, lo, hi in due:
                parts.setdefault(u, []).append((emb[u, lo:hi], near[u, lo:hi], dmin[u, lo:hi], dist[u, lo:hi, :N]))
        cat = lambda p: p[0] if len(p) == 1 else torch.cat(p, dim=0)
        return {u: EmbedResult(*(cat(f) for f in zip(*p))) for u, p in parts.items()}
