"""What a decoder or an aligner hands on, from the class track of ``BatchedFSM.classpath`` (mm_classpath_f32): the sequence of
labels with their times (``events``), the runs between boundary arcs (``segments``), and forced alignment under partial time marks
(``forced_alignment``: the marks become 0 / -inf class scores, ``transitions.constraint_scores``).

A class track is ``classes[B, N]``: ``classes[b, t]`` is the class of the entry the best path of utterance b takes between frames t
and t + 1 (0-based; t = len - 1: the arc into the phony final state), -1 for an unclassified entry, beyond the length and where
there is no path.

And from the ``Lattice`` of ``BatchedFSM.lattice`` (mm_lattice_f32): one utterance's kept arcs as host arrays (``lattice_arcs``) and
as an acyclic tropical FSM that goes back into ``compile`` / ``batch`` for rescoring (``lattice_fsm``); and the lattice of the
records above a posterior threshold (``lattice_prune``, on the posteriors of ``BatchedFSM.latticeposteriors``).  After a rescoring
(``BatchedFSM.latticebest``, mm_latticebest_f32): the lattice re-pruned to a beam under the new scores (``lattice_rescore``) and one
utterance's new best path as host arrays (``lattice_onebest``).
"""
from __future__ import annotations

import numpy as np

from .fsm import FSM, _entry_ends
from .transitions import constraint_scores


def _host(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def events(classes, lens, ignore=(-1,)):
    """Per utterance the list of ``(class, t)`` at which the path takes an entry whose class is not in ``ignore``: the label
    sequence with its times.  ``classes`` [B, N] ints, ``lens`` [B]."""
    cls, lens = _host(classes), _host(lens)
    skip = set(int(c) for c in ignore)
    return [[(int(c), t) for t, c in enumerate(cls[b, : int(lens[b])]) if int(c) not in skip] for b in range(cls.shape[0])]


def segments(classes, lens, boundary):
    """Per utterance the list of ``(start, end)`` frame runs (0-based, end exclusive) that the arcs of class ``boundary`` cut the
    frames 0 .. len-1 into: a boundary arc at transition t ends a run behind frame t, the next starts at frame t + 1.  The arc
    into the final state (t = len - 1) ends the last run whatever its class; an utterance without a path (a track of -1 with
    len > 0 included) still gives the one run (0, len); len = 0 gives none."""
    cls, lens = _host(classes), _host(lens)
    out = []
    for b in range(cls.shape[0]):
        n, runs, start = int(lens[b]), [], 0
        for t in range(n):
            if t == n - 1 or int(cls[b, t]) == int(boundary):
                runs.append((start, t + 1))
                start = t + 1
        out.append(runs)
    return out


def forced_alignment(bf, V, marks, lens=None):
    """Best paths under partial time marks: ``marks[b]`` is a list of ``(t, class)`` -- at transition t (between frames t and t + 1,
    0-based) the path of utterance b takes an entry of that class, or an unclassified one: every other class gets the score -inf
    there, everything else 0.  ``bf`` is a tropical batch with its classes set (``set_path_classes``); ``V`` and ``lens`` as for
    ``classpath``.  Returns ``classpath``'s ``(path, classes, score)``; an utterance whose marks no path can meet has score -inf."""
    info = bf.path_class_info()
    nc = info["path_C"]
    if nc < 1:
        raise ValueError("forced_alignment: no classes set (set_path_classes)")
    B, N = int(V.shape[0]), int(V.shape[1])
    if len(marks) != B:
        raise ValueError(f"forced_alignment: {len(marks)} mark lists for a batch of {B}")
    allowed = np.ones((B, N, nc), dtype=np.bool_)
    for b, ms in enumerate(marks):
        for t, c in ms:
            if not (0 <= int(t) < N and 0 <= int(c) < nc):
                raise ValueError(f"forced_alignment: mark ({t}, {c}) of utterance {b} is outside [0, {N}) x [0, {nc})")
            keep = allowed[b, int(t), int(c)]
            allowed[b, int(t), :] = False
            allowed[b, int(t), int(c)] = keep  # (two different marks at one transition: nothing is allowed)
    return bf.classpath(V, constraint_scores(allowed), lens)


def lattice_arcs(bf, lat, b):
    """One utterance of a ``Lattice`` (``BatchedFSM.lattice``) on the host: the arrays ``(t, arc, src, dst, score)`` of its records in
    their order -- the transition (0-based; the last one holds the arcs into the phony final state), the stored entry k of the
    utterance's FSM (the order of ``FSM.nzval``), its source and destination state, and its through-score relative to the best path."""
    counts, offsets, arc, score = _host(lat.counts), _host(lat.offsets), _host(lat.arc), _host(lat.score)
    N = counts.shape[1]
    lo, hi = int(offsets[b * N]), int(offsets[(b + 1) * N])
    if hi > arc.shape[0]:
        raise ValueError(f"lattice_arcs: utterance {b} ends at record {hi}, the lattice holds {arc.shape[0]} (max_arcs cut it)")
    k = arc[lo:hi].astype(np.int64)
    src, dst = _entry_ends(bf.cfsms[b].fsm)
    return np.repeat(np.arange(N, dtype=np.int64), counts[b]), k, src[k], dst[k], score[lo:hi].copy()


def lattice_fsm(bf, lat, b):
    """One utterance of a ``Lattice`` as a graph: ``(fsm, state2pdf)``, a tropical ``FSM`` whose states are the (frame, state) pairs
    the kept arcs touch, in (frame, state) order and labelled so -- acyclic, a state of frame n is only ever visited at frame n, so
    with ``state2pdf`` (the original state's pdf) it reads the SAME ``V`` and goes straight back into ``compile`` / ``batch``:
    ``bestpath`` on it returns the original best score, and a second model's ``V`` rescores the pruned space.  The initial weights
    are the alpha_hat of the sources of transition 0, the final weights the weights of the arcs into the phony final state, every
    other kept arc keeps its weight (parallel entries merge into their maximum).  An utterance without a path has no lattice:
    ValueError."""
    t, k, src, dst, _ = lattice_arcs(bf, lat, b)
    if k.size == 0:
        raise ValueError(f"lattice_fsm: utterance {b} has no arc within the beam")
    cf = bf.cfsms[b]
    f, S1 = cf.fsm, cf.S1
    w = np.asarray(f.nzval, dtype=np.float32)[k]
    last = t == t.max()  # (the arcs into the phony final state)
    keys = np.unique(np.concatenate([t * S1 + src, (t[~last] + 1) * S1 + dst[~last]]))
    node = lambda frame, state: np.searchsorted(keys, frame * S1 + state)
    a_hat = dict(zip((int(s) for s in f.alpha_idx), (float(v) for v in f.alpha_val)))
    first = np.unique(src[t == 0])
    initws = [(int(node(0, s)), a_hat[int(s)]) for s in first]
    a, c = node(t[~last], src[~last]), node(t[~last] + 1, dst[~last])
    arcs = [((int(x), int(y)), float(v)) for x, y, v in zip(a, c, w[~last])]
    finalws = [(int(x), float(v)) for x, v in zip(node(t[last], src[last]), w[last])]
    labels = [(int(q // S1), int(q % S1)) for q in keys]
    s2p = np.asarray(cf.C_hat.state2pdf, dtype=np.int64)[keys % S1]
    return FSM(initws, arcs, finalws, labels, semiring="tropical", dtype=np.float32), s2p


def lattice_prune(lat, post, threshold):
    """Posterior pruning of a ``Lattice``: the ``Lattice`` of the records with ``post >= log(threshold)``, ``post`` being the record
    log posteriors of ``BatchedFSM.latticeposteriors`` on ``lat`` and ``threshold`` a probability (0 keeps every record with a path
    through it).  Counts and offsets are recomputed, ``arc`` and ``score`` keep their order, ``best`` stays: the result goes back into
    ``latticeposteriors``, ``lattice_arcs`` and ``lattice_fsm``.  Tensor members stay tensors on their device (no host
    synchronisation but the one that sizes the result), NumPy members stay NumPy."""
    import math

    n = lat.arc.shape[0]
    if post.shape[0] != n or lat.score.shape[0] != n:
        raise ValueError(f"lattice_prune: {post.shape[0]} posteriors and {lat.score.shape[0]} scores for {n} records")
    if threshold < 0:
        raise ValueError(f"lattice_prune: threshold must be a probability, got {threshold}")
    bound = math.log(threshold) if threshold > 0 else -math.inf
    B, N = lat.counts.shape
    if hasattr(lat.arc, "cpu"):  # (tensors)
        import torch

        offsets = lat.offsets.to(lat.arc.device)
        keep = post.to(lat.arc.device) >= bound
        if threshold <= 0:
            keep &= ~torch.isneginf(post.to(lat.arc.device))
        r = torch.arange(n, device=lat.arc.device, dtype=offsets.dtype)
        cell = torch.searchsorted(offsets[1:].contiguous(), r, right=True)
        keep &= cell < B * N  # (records behind the last cell belong to no transition)
        counts = torch.bincount(cell[keep], minlength=B * N)[: B * N].to(lat.counts.dtype).reshape(B, N)
        offs = torch.cat([torch.zeros(1, dtype=offsets.dtype, device=offsets.device), torch.cumsum(counts.reshape(-1), 0, dtype=offsets.dtype)])
        return type(lat)(counts, offs, lat.arc[keep], lat.score[keep], lat.best)
    offsets, p = _host(lat.offsets), _host(post)
    keep = p >= bound
    if threshold <= 0:
        keep &= ~np.isneginf(p)
    cell = np.searchsorted(offsets[1:], np.arange(n, dtype=np.int64), side="right")
    keep &= cell < B * N
    counts = np.bincount(cell[keep], minlength=B * N)[: B * N].astype(_host(lat.counts).dtype).reshape(B, N)
    offs = np.concatenate([[0], np.cumsum(counts.reshape(-1), dtype=np.int64)])
    return type(lat)(counts, offs, _host(lat.arc)[keep], _host(lat.score)[keep], lat.best)


def lattice_rescore(bf, lat, V, extra=None, lens=None, beam=None):
    """A ``Lattice`` under new scores: ``BatchedFSM.latticebest`` on ``lat`` with the emissions ``V`` and the per-record scores
    ``extra`` (a language model's, say), then the ``Lattice`` of the records whose NEW through-score is within ``beam`` of the new
    best path (``score >= -beam``; ``beam`` None: every record with a finite score), with the new ``score`` and ``best``.  Counts and
    offsets are recomputed as ``lattice_prune`` does, ``arc`` keeps its order: the result goes back into every entry that reads a
    lattice.  On the lattice's own ``V`` with ``extra`` None and exact inputs this is the lattice ``bf.lattice`` returns at the
    narrower beam.  Tensors stay on the device (one synchronisation, the one that sizes the result); NumPy in, NumPy out."""
    if beam is not None and not beam >= 0:
        raise ValueError(f"lattice_rescore: beam must be >= 0 or None, got {beam}")
    res = bf.latticebest(lat, V, lens, extra, want_path=False)
    n = res.score.shape[0]
    B, N = lat.counts.shape
    if hasattr(res.score, "cpu"):  # (tensors)
        import torch

        dev = res.score.device
        offsets = torch.as_tensor(lat.offsets).to(dev)
        keep = ~torch.isneginf(res.score) if beam is None else res.score >= -float(beam)
        cell = torch.searchsorted(offsets[1:].contiguous(), torch.arange(n, device=dev, dtype=offsets.dtype), right=True)
        keep &= cell < B * N  # (records behind the last cell belong to no transition)
        counts = torch.bincount(cell[keep], minlength=B * N)[: B * N].to(torch.int32).reshape(B, N)
        offs = torch.cat([torch.zeros(1, dtype=offsets.dtype, device=dev), torch.cumsum(counts.reshape(-1), 0, dtype=offsets.dtype)])
        return type(lat)(counts, offs, torch.as_tensor(lat.arc).to(dev)[keep], res.score[keep], res.best)
    offsets = _host(lat.offsets)
    keep = ~np.isneginf(res.score) if beam is None else res.score >= -np.float32(beam)
    cell = np.searchsorted(offsets[1:], np.arange(n, dtype=np.int64), side="right")
    keep &= cell < B * N
    counts = np.bincount(cell[keep], minlength=B * N)[: B * N].astype(np.int32).reshape(B, N)
    offs = np.concatenate([[0], np.cumsum(counts.reshape(-1), dtype=np.int64)])
    return type(lat)(counts, offs, _host(lat.arc)[keep], res.score[keep], res.best)


def lattice_onebest(bf, lat, res, b):
    """Utterance b's best path through the lattice ``lat`` as ``BatchedFSM.latticebest`` found it (``res``, asked for with its
    path), on the host: the arrays ``(t, arc, src, dst)`` of its records, one per transition -- ``lattice_arcs``' columns without
    the score.  Empty arrays for an utterance without a path."""
    if res.rec is None:
        raise ValueError("lattice_onebest: the LatticeBest holds no path (want_path=False)")
    r = _host(res.rec)[b].astype(np.int64)
    r = r[r >= 0]
    k = _host(lat.arc)[r].astype(np.int64)
    src, dst = _entry_ends(bf.cfsms[b].fsm)
    return np.arange(r.size, dtype=np.int64), k, src[k], dst[k]
