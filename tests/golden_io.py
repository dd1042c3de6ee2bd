"""Fixtures of tests/golden/ that would exceed the repository's 1 MiB limit for a committed file are stored in two parts:
tests/golden/<name>.npz and tests/golden/more/<name>.npz, each holding some of the arrays. load() joins them, save() splits."""
from __future__ import annotations

import io
import os

import numpy as np

LIMIT = 1_000_000          # bytes per file, below 1 MiB


def _more(path):
    return os.path.join(os.path.dirname(path), "more", os.path.basename(path))


def load(path) -> dict:
    g = dict(np.load(path))
    if os.path.exists(_more(path)):
        g.update(np.load(_more(path)))
    return g


def _size(arrays) -> int:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(path, **arrays):
    """np.savez_compressed; when the file would exceed LIMIT, the largest arrays go to more/<name>.npz"""
    main, rest = dict(arrays), {}
    while _size(main) > LIMIT:
        big = max(main, key=lambda k: np.asarray(main[k]).nbytes)
        rest[big] = main.pop(big)
    np.savez_compressed(path, **main)
    if rest:
        assert _size(rest) <= LIMIT, "fixture too large even in two parts"
        os.makedirs(os.path.dirname(_more(path)), exist_ok=True)
        np.savez_compressed(_more(path), **rest)
    elif os.path.exists(_more(path)):
        os.unlink(_more(path))
