"""What a decoder or an aligner hands on, from the class track of ``BatchedFSM.classpath`` (mm_classpath_f32): the sequence of
labels with their times (``events``), the runs between boundary arcs (``segments``), and forced alignment under partial time marks
(``forced_alignment``: the marks become 0 / -inf class scores, ``transitions.constraint_scores``).

A class track is ``classes[B, N]``: ``classes[b, t]`` is the class of the entry the best path of utterance b takes between frames t
and t + 1 (0-based; t = len - 1: the arc into the phony final state), -1 for an unclassified entry, beyond the length and where
there is no path.
"""
from __future__ import annotations

import numpy as np

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
