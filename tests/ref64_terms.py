"""Replays of what the terms of a mesh share behind their per-element kernels (zpc_amd/csrc/mesh_terms.hip), numpy only, in the device's
order: the incidence by vertex, the per-vertex gather over one or more runs and the float64 total of the float32 energies."""
import numpy as np


def incidence(elems, nv):
    """(starts [nv + 1], entries): the numbers N element + corner of the corners of elems [n, N] stably sorted by vertex; a corner whose
    vertex is outside [0, nv) is in no run"""
    flat = np.asarray(elems, np.int64).reshape(-1)
    keep = np.flatnonzero((flat >= 0) & (flat < nv))
    order = keep[np.argsort(flat[keep], kind="stable")]
    return np.searchsorted(flat[order], np.arange(nv + 1)), order


def gather(nv, runs, dtype):
    """out [nv, ...]: for every vertex the sum of terms[entries] over its runs, one run after the other, each front to back, added one at
    a time in dtype.  runs: a list of (starts, entries, terms [n * N, ...])"""
    out = None
    for starts, entries, terms in runs:
        terms = np.asarray(terms, dtype)
        if out is None:
            out = np.zeros((nv,) + terms.shape[1:], dtype)
        deg = np.diff(starts)
        for k in range(int(deg.max()) if len(deg) else 0):
            v = np.nonzero(deg > k)[0]
            out[v] = out[v] + terms[entries[starts[v] + k]]
    return out


def total(energies):
    """the float64 sum of float32 energies in the order of terms_partial_kernel / terms_total_kernel: workgroup g takes elements
    [4096 g, 4096 (g + 1)), thread t of 256 the elements t, t + 256, ..; then an LDS tree; one workgroup sums the partials the same way"""
    def block(a, chunk):
        pad = np.zeros(chunk, np.float64)
        pad[:len(a)] = a
        s = np.zeros(256)
        for row in pad.reshape(-1, 256):
            s = s + row
        h = 128
        while h:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
        return s[0]
    a = np.asarray(energies, np.float32).astype(np.float64)
    parts = np.array([block(a[i:i + 4096], 4096) for i in range(0, len(a), 4096)])
    return block(parts, 256 * max(1, -(-len(parts) // 256)))
