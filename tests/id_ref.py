"""The expected material-ID records (include/rt.h rt_render_ids), composed on the CPU.

Per-sample ids: the material column of pyoracle.closest_hits over tests/feature_ref.py's primary rays (first hit),
or the material of the terminal vertex of the specular chain, stepped here with tests/feature_chain_ref.py's own
pieces (its streams, its Dielectric and Metal scatters, its undecided margin; its Chain keeps how a chain ended and
not where, so the loop is restated, and tests/test_ids_host.py checks the restatement's counts against Chain's).
Then rt.h's fold, restated in Python. Worlds without media only, for the reason feature_ref gives.

Shared by the host and the GPU tests; compositions are cached and must be left unchanged."""
import functools

import numpy as np

import feature_chain_ref as fcr
import feature_ref
import pyoracle
import rtamd

MISS = 0xFFFFFFFF
SLOTS = 7
ID_DTYPE = np.dtype([("id", "<u4", (SLOTS,)), ("count", "<u4", (SLOTS,)), ("other", "<u4"), ("samples", "<u4")])


def fold(ids, rec=None):
    """rt.h's fold of the sample ids `ids`, in order, into a copy of `rec` ((id list, count list, other, samples);
    None: the zero record)."""
    sid, cnt, other, samples = ([0] * SLOTS, [0] * SLOTS, 0, 0) if rec is None else (list(rec[0]), list(rec[1]), rec[2], rec[3])
    for x in ids:
        if samples == 0xFFFFFFFF:
            continue
        used = [k for k in range(SLOTS) if cnt[k] > 0 and sid[k] == x]
        free = [k for k in range(SLOTS) if cnt[k] == 0]
        if used:
            cnt[used[0]] += 1
        elif free:
            sid[free[0]], cnt[free[0]] = int(x), 1
        else:
            other += 1
        samples += 1
    return sid, cnt, other, samples


def as_tuple(rec):
    """A numpy record (0-d array or void of ID_DTYPE) as fold's tuple."""
    r = np.asarray(rec).reshape(())
    return [int(v) for v in r["id"]], [int(v) for v in r["count"]], int(r["other"]), int(r["samples"])


def as_record(t):
    r = np.zeros((), dtype=ID_DTYPE)
    r["id"], r["count"], r["other"], r["samples"] = t[0], t[1], t[2], t[3]
    return r


def records(ids, first=0, n=None, start=None):
    """Per-sample ids (n_all, H, W) folded per pixel over samples first .. first + n - 1 of the array (default: to
    its end), from zero records or from `start` (H, W): (H, W) of ID_DTYPE."""
    n_all, H, W = ids.shape
    n = n_all - first if n is None else n
    out = np.zeros((H, W), dtype=ID_DTYPE)
    for r in range(H):
        for c in range(W):
            rec = None if start is None else as_tuple(start[r, c])
            out[r, c] = as_record(fold(ids[first:first + n, r, c].tolist(), rec))[()]
    return out


@functools.lru_cache(maxsize=None)
def first_hit_ids(name, W, H, n, seed=1024, first=0):
    """(n, H, W) uint32: the material each sample's primary ray hits first, MISS for the background."""
    scene, cam = fcr.world(name)
    rays = feature_ref.primary_rays(cam(W, H), W, H, seed, range(first, first + n))
    hits = pyoracle.closest_hits(scene, rays.reshape(-1, 7), 1e-4, float("inf"))
    ids = np.where(hits[:, 0] == 1, hits[:, 11], float(MISS)).astype(np.uint32).reshape(n, H, W)
    ids.setflags(write=False)
    return ids


class ChainIds:
    """ids (n, H, W) uint32: the material of each sample's terminal vertex (MISS: the chain ended in a miss);
    left_out (H, W): pixels with an undecided sample; counts(): rt_feature_chain_stats of the pass."""

    def __init__(self, scene, cam, W, H, seed, first, n, max_bounces, flags, max_fuzz):
        d = scene.desc
        assert not any(d.nodes[i].type == rtamd.RT_NODE_CONSTANT_MEDIUM for i in range(d.n_nodes)), "no media here"
        mtype = np.array([d.materials[m].type for m in range(d.n_materials)])
        mparam = np.array([d.materials[m].param for m in range(d.n_materials)])
        rays, g = fcr.primary_rays_and_streams(cam, W, H, seed, range(first, first + n))
        N = len(rays)
        ids = np.full(N, MISS, dtype=np.uint32)
        kind, b = np.full(N, -1), np.zeros(N, dtype=np.int64)
        undecided = np.zeros(N, dtype=bool)
        active = np.ones(N, dtype=bool)
        while active.any():
            idx = np.flatnonzero(active)
            hits = pyoracle.closest_hits(scene, rays[idx], 1e-4, float("inf"))
            got = hits[:, 0] == 1
            kind[idx[~got]] = fcr.MISS
            active[idx[~got]] = False
            idx, hits = idx[got], hits[got]
            mats = hits[:, 11].astype(np.int64)
            diel, metal = mtype[mats] == fcr.RT_MAT_DIELECTRIC, mtype[mats] == fcr.RT_MAT_METAL
            could = (diel & bool(flags & fcr.RT_CHAIN_DIELECTRIC)) | (metal & bool(flags & fcr.RT_CHAIN_METAL) &
                                                                      (mparam[mats] <= max_fuzz))
            follow = could & (b[idx] < max_bounces)
            end = idx[~follow]
            ids[end] = mats[~follow]
            kind[end] = np.where(could[~follow], fcr.CAP, fcr.SURFACE)
            active[end] = False
            dd = rays[idx, 3:6]
            new_d = np.zeros((len(idx), 3))
            m_sel, d_sel = follow & metal, follow & diel
            if m_sel.any():  # Metal draws two words, Dielectric one
                mask = np.zeros(N, dtype=bool)
                mask[idx[m_sel]] = True
                aa, zz = g.draw(mask), g.draw(mask)
                new_d[m_sel] = fcr.scatter_metal(dd[m_sel], hits[m_sel, 5:8], mparam[mats[m_sel]], aa, zz)
            if d_sel.any():
                mask = np.zeros(N, dtype=bool)
                mask[idx[d_sel]] = True
                rd = g.draw(mask)
                new_d[d_sel], margin = fcr.scatter_dielectric(dd[d_sel], hits[d_sel, 5:8], hits[d_sel, 10],
                                                              mparam[mats[d_sel]], rd)
                undecided[idx[d_sel]] |= margin < fcr.UNDECIDED
            go = idx[follow]
            rays[go, 0:3] = hits[follow, 2:5]
            rays[go, 3:6] = new_d[follow]
            b[go] += 1
        self.ids = ids.reshape(n, H, W)
        self.kind, self.bounces = kind.reshape(n, H, W), b.reshape(n, H, W)
        self.left_out = undecided.reshape(n, H, W).any(axis=0)
        for a in (self.ids, self.kind, self.bounces, self.left_out):
            a.setflags(write=False)

    def counts(self):
        return dict(samples=int(self.kind.size), ended_surface=int((self.kind == fcr.SURFACE).sum()),
                    ended_miss=int((self.kind == fcr.MISS).sum()), ended_cap=int((self.kind == fcr.CAP).sum()),
                    bounces=int(self.bounces.sum()))


@functools.lru_cache(maxsize=None)
def chain_ids(name, W, H, n, max_bounces, flags, max_fuzz=0.0, seed=1024, first=0):
    scene, cam = fcr.world(name)
    return ChainIds(scene, cam(W, H), W, H, seed, first, n, max_bounces, flags, max_fuzz)


@functools.lru_cache(maxsize=None)
def first_hit_records(name, W, H, n, seed=1024):
    """The records of a pass without a chain over samples 0 .. n - 1; read-only."""
    out = records(first_hit_ids(name, W, H, n, seed))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def chain_records(name, W, H, n, max_bounces, flags, max_fuzz=0.0, seed=1024):
    out = records(chain_ids(name, W, H, n, max_bounces, flags, max_fuzz, seed).ids)
    out.setflags(write=False)
    return out
