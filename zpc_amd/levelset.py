"""Sparse level sets: zs::LevelSetBoundary<SparseGrid<3, f32, 8>> (geometry/Collider.h:246-252, geometry/SparseGrid.hpp) built from a
dense signed-distance array -- a bht<int, 3, int, 16> keyed by block origins next to a TileVector<f32, 512> with the properties "sdf"
(1 channel) and optionally "v" (3 channels) -- for MpmTransfer.apply_boundary / implicit_project / implicit_solve / step_slotted
(levelset=), and LevelSetSequence, the queue of keyframes whose two front entries those calls blend (an animated collider rebuilt once
per frame instead of once per sub-step).  Set-up code: numpy and torch for the plumbing, the library's containers for the storage."""
import ctypes as C

import numpy as np

from ._lib import lib, LevelSet, LevelSetTransition
from .containers import Bht, TileVector

SIDE, BLOCK = 8, 512   # SparseGrid<3, f32, 8>


def select_blocks(sdf, band, background, vel=None):
    """Host part of from_dense (no device needed): the 8^3 blocks of the dense array `sdf` [nx, ny, nz] (cell (i, j, k) = level-set
    index (i, j, k); the array is padded with `background` up to multiples of 8) that hold a cell with |sdf| < band.
    Returns (keys [nb, 3] int32 block origins in lexicographic order, cells [nb * 512, C] float32 with C = 1 or 4: sdf, v)."""
    sdf = np.asarray(sdf, np.float32)
    if sdf.ndim != 3:
        raise ValueError("sdf: a dense [nx, ny, nz] array")
    chans = [sdf]
    if vel is not None:
        vel = np.asarray(vel, np.float32)
        if vel.shape != sdf.shape + (3,):
            raise ValueError("vel: [nx, ny, nz, 3]")
        chans += [vel[..., d] for d in range(3)]
    nb3 = [(n + SIDE - 1) // SIDE for n in sdf.shape]
    padded = np.full([len(chans)] + [n * SIDE for n in nb3], np.float32(background), np.float32)
    for c, a in enumerate(chans):
        padded[c, :sdf.shape[0], :sdf.shape[1], :sdf.shape[2]] = a
    # [C, bx, 8, by, 8, bz, 8] -> [bx, by, bz, 8, 8, 8, C]: cell offset (x * 8 + y) * 8 + z inside a block, first axis slowest
    tiles = padded.reshape(len(chans), nb3[0], SIDE, nb3[1], SIDE, nb3[2], SIDE).transpose(1, 3, 5, 2, 4, 6, 0)
    active = (np.abs(tiles[..., 0]) < np.float32(band)).any(axis=(3, 4, 5))
    idx = np.argwhere(active)
    keys = (idx * SIDE).astype(np.int32)
    cells = np.ascontiguousarray(tiles[active]).reshape(-1, len(chans))
    return keys, cells


class SparseLevelSet:
    """A level set on the device.  index = (world - origin) / voxel; cells of blocks that are not stored read as `background`."""

    def __init__(self, pol, keys, cells, origin, voxel, background):
        import torch
        self.pol = pol
        self.keys = np.ascontiguousarray(keys, np.int32)
        nb = self.keys.shape[0]
        nch = cells.shape[1]
        if nch not in (1, 4):
            raise ValueError("cells: [nb * 512, 1] (sdf) or [nb * 512, 4] (sdf, v)")
        self.has_velocity = nch == 4
        self.nblocks = nb
        self.origin = tuple(float(v) for v in origin)
        self.voxel, self.background = float(voxel), float(background)
        self.table = Bht(3, max(nb, 1), bucket=16)
        tags = [("sdf", 1)] + ([("v", 3)] if self.has_velocity else [])
        self.tiles = TileVector("float", BLOCK, tags, max(nb, 1) * BLOCK)
        if nb:
            dk = torch.from_numpy(self.keys).cuda()
            self.table.assign(pol, dk.data_ptr(), nb)   # block number = position in `keys`
            dc = torch.from_numpy(np.ascontiguousarray(cells, np.float32)).cuda()
            lib().zs_rocm_tv_from_aos_f32(pol.handle, dc.data_ptr(), nb * BLOCK, nch, BLOCK, self.tiles.data())
            pol.syncCtx()
        self.stats = None
        self.band = None   # set by from_dense / from_mesh (update_from_mesh needs it)
        self._make_view()

    def _make_view(self):
        v = LevelSet()
        v.table = self.table.view()
        v.tiles = self.tiles.data()
        v.numBlocks = self.nblocks
        v.numChannels = self.tiles.numChannels()
        v.sdfChannel = self.tiles.getPropertyOffset("sdf")
        v.velChannel = self.tiles.getPropertyOffset("v") if self.has_velocity else -1
        v.h = self.voxel
        v.origin = (C.c_float * 3)(*self.origin)
        v.background = self.background
        v.stats = self.stats.data_ptr() if self.stats is not None else None
        self.view = v

    @classmethod
    def from_dense(cls, pol, sdf, origin, voxel, band, vel=None, background=None):
        """sdf: dense numpy / torch array [nx, ny, nz], cell (0, 0, 0) at world `origin`, spacing `voxel`; every 8^3 block holding a
        cell with |sdf| < band is stored.  vel: optional [nx, ny, nz, 3] material velocity.  background defaults to band."""
        to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        background = band if background is None else background
        keys, cells = select_blocks(to_np(sdf), band, background, None if vel is None else to_np(vel))
        self = cls(pol, keys, cells, origin, voxel, background)
        self.band = float(band)
        return self

    @classmethod
    def from_function(cls, pol, fn, lo, hi, voxel, band, vel_fn=None, background=None):
        """fn(x [..., 3] float64 world positions) -> signed distance, sampled on the lattice lo + voxel * (i, j, k) that covers [lo, hi]"""
        lo = np.asarray(lo, np.float64)
        n = [int(np.ceil((h - l) / voxel)) + 1 for l, h in zip(lo, hi)]
        x = lo + voxel * np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1)
        return cls.from_dense(pol, fn(x), lo, voxel, band, vel=None if vel_fn is None else vel_fn(x), background=background)

    @classmethod
    def from_mesh(cls, pol, mesh, voxel, band, origin=None, background=None, allow_open=False):
        """The level set of a TriMesh, built on the device: what from_dense makes of the mesh's signed distance sampled at
        origin + voxel * (i, j, k) -- every 8^3 block with a cell |sdf| < band, all 512 cells of it the signed distance, blocks numbered in
        lexicographic key order; with vertex velocities the tiles carry "v".  origin defaults to the mesh's total box minus band, snapped
        down to a multiple of voxel; background defaults to band.  The host only sizes the containers."""
        from .mesh import default_origin
        if not (voxel > 0 and band > 0):
            raise ValueError("from_mesh: voxel and band must be positive")
        if not allow_open and not mesh.is_closed():
            raise ValueError("from_mesh: the mesh is not closed and consistently oriented (%r); pass allow_open=True to take the "
                             "pseudonormal sign anyway" % (mesh.stats(),))
        if origin is None:
            origin = default_origin(mesh.total_box()[0], voxel, band)
        self = cls.__new__(cls)
        self.pol = pol
        self.origin = tuple(float(v) for v in origin)
        self.voxel, self.band = float(voxel), float(band)
        self.background = float(band if background is None else background)
        self.has_velocity = bool(mesh.has_velocity)
        self.stats = None
        self.build_stats = None
        self.update_from_mesh(mesh)
        return self

    def update_from_mesh(self, mesh):
        """rebuild in place from the mesh's current vertices (after TriMesh.refit): same origin, voxel, band and channels"""
        import torch
        from .mesh import candidate_capacity
        L, pol = lib(), self.pol
        if bool(mesh.has_velocity) != self.has_velocity:
            raise ValueError("update_from_mesh: the mesh's velocities must stay present / absent")
        nch = 4 if self.has_velocity else 1
        org = (C.c_float * 3)(*self.origin)
        if getattr(self, "band", None) is None:
            raise ValueError("update_from_mesh: this level set does not know its band (built from keys and cells directly)")
        voxel, band = self.voxel, self.band
        nkept, keys = 0, np.zeros((0, 3), np.int32)
        self.build_stats = np.zeros(4, np.int64)
        if mesh.nt:
            pairs = L.zs_rocm_mesh_levelset_count(pol.handle, mesh.handle, org, voxel, band)
            if pairs == C.c_size_t(-1).value:
                raise ValueError("from_mesh: the lattice is too fine for this mesh (2^31 candidate blocks or more)")
            lo, hi = mesh.total_box()
            cand = Bht(3, candidate_capacity(pairs, lo, hi, self.origin, voxel, band), bucket=16)
            if L.zs_rocm_mesh_levelset_candidates(pol.handle, mesh.handle, org, voxel, band, cand.handle) != 0:
                raise RuntimeError("zs_rocm_mesh_levelset_candidates failed")
            pol.syncCtx()
            ncand = cand.size()
            if not cand.success():
                raise RuntimeError("from_mesh: the candidate table overflowed")
            scratch = torch.empty(max(ncand, 1) * nch * BLOCK, dtype=torch.float32, device="cuda")
            keep = torch.zeros(max(ncand, 1), dtype=torch.int32, device="cuda")
            stats = torch.zeros(4, dtype=torch.int32, device="cuda")
            if L.zs_rocm_mesh_levelset_blocks(pol.handle, mesh.handle, org, voxel, band, cand.handle, ncand, scratch.data_ptr(), nch,
                                              keep.data_ptr(), stats.data_ptr()) != 0:
                raise RuntimeError("zs_rocm_mesh_levelset_blocks failed")
            kept = torch.empty(max(ncand, 1), 3, dtype=torch.int32, device="cuda")
            nkept = L.zs_rocm_mesh_levelset_select(pol.handle, cand.handle, ncand, keep.data_ptr(), kept.data_ptr())
            if nkept == C.c_size_t(-1).value:
                raise RuntimeError("zs_rocm_mesh_levelset_select failed")
            self.build_stats = stats.cpu().numpy().astype(np.int64)
        self.nblocks = int(nkept)
        self.table = Bht(3, max(self.nblocks, 1), bucket=16)
        tags = [("sdf", 1)] + ([("v", 3)] if self.has_velocity else [])
        self.tiles = TileVector("float", BLOCK, tags, max(self.nblocks, 1) * BLOCK)
        if self.nblocks:
            self.table.insert(pol, kept.data_ptr(), self.nblocks)
            self.table.canonicalize(pol)   # lexicographic key order: the numbering select_blocks gives
            if L.zs_rocm_mesh_levelset_gather(pol.handle, cand.handle, ncand, keep.data_ptr(), scratch.data_ptr(), self.table.handle,
                                              self.tiles.data(), nch) != 0:
                raise RuntimeError("zs_rocm_mesh_levelset_gather failed")
            pol.syncCtx()
            keys = self.active_keys()
        self.keys = keys
        self._make_view()

    def active_keys(self):
        """the block origins in block-number order, read back from the table [nblocks, 3]"""
        a = np.empty((self.nblocks, 3), np.int32)
        if self.nblocks:
            C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(self.table.view().activeKeys), C.c_size_t(a.nbytes), 2)
        return a

    def max_speed(self):
        """the largest |v_d| over the three "v" channels of all cells of all stored blocks (get_level_set_max_speed,
        geometry/LevelSetUtils.tpp), 0.0 without "v"; reduced on the device, synchronises the stream"""
        import torch
        out = torch.empty(1, dtype=torch.float32, device="cuda")
        if lib().zs_rocm_levelset_max_speed(self.pol.handle, C.byref(self.view), out.data_ptr()) != 0:
            raise RuntimeError("zs_rocm_levelset_max_speed refused its arguments")
        self.pol.syncCtx()
        return float(out.item())

    def enable_stats(self):
        """count, per block-kernel launch and grid block, how the block was handled: stats()[0] culled, [1] staged, [2] direct"""
        import torch
        self.stats = torch.zeros(4, dtype=torch.int32, device="cuda")
        self._make_view()

    def read_stats(self, reset=True):
        self.pol.syncCtx()
        s = self.stats.cpu().numpy().astype(np.int64)
        if reset:
            self.stats.zero_()
        return s

    def to_dense(self, lo, hi):
        """the cells of the index-space box [lo, hi) as a dense array [.., .., .., C] (C = 1 or 4), background where no block is stored;
        read back from the device: block numbers through the table, values from the tiles"""
        import torch
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        nch = 4 if self.has_velocity else 1
        out = np.full(tuple(hi - lo) + (nch,), np.float32(self.background), np.float32)
        if not self.nblocks:
            return out
        aos = torch.empty(self.nblocks * BLOCK, nch, dtype=torch.float32, device="cuda")
        lib().zs_rocm_tv_to_aos_f32(self.pol.handle, self.tiles.data(), self.nblocks * BLOCK, nch, BLOCK, aos.data_ptr())
        blo, bhi = lo // SIDE, (hi + SIDE - 1) // SIDE
        bk = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(blo, bhi)], indexing="ij"), axis=-1).reshape(-1, 3)
        q = torch.from_numpy(np.ascontiguousarray(bk * SIDE, np.int32)).cuda()
        bno = torch.empty(q.shape[0], dtype=torch.int32, device="cuda")
        self.table.query(self.pol, q.data_ptr(), q.shape[0], bno.data_ptr())
        self.pol.syncCtx()
        tiles = aos.cpu().numpy().reshape(self.nblocks, SIDE, SIDE, SIDE, nch)
        for k, b in zip(bk, bno.cpu().numpy()):
            if b < 0:
                continue
            o = k * SIDE
            a, e = np.maximum(o, lo), np.minimum(o + SIDE, hi)
            if (a < e).all():
                out[a[0] - lo[0]:e[0] - lo[0], a[1] - lo[1]:e[1] - lo[1], a[2] - lo[2]:e[2] - lo[2]] = \
                    tiles[b, a[0] - o[0]:e[0] - o[0], a[1] - o[1]:e[1] - o[1], a[2] - o[2]:e[2] - o[2]]
        return out


POP_THRESHOLD = np.float32(1) - np.float32(128) * np.finfo(np.float32).eps


class LevelSetSequence:
    """The keyframe queue of the reference's ConstTransitionLevelSetPtr (geometry/LevelSet.h): push(level set) appends a keyframe, the two
    front ones are blended at the phase alpha (TransitionLevelSetView, include/zensim_rocm/levelset_device.hpp), advance(ratio) moves
    the phase and drops the front keyframe each time it passes 1.  step_dt: the time between two keyframes.  Pass the sequence (or its
    view()) as levelset= to MpmTransfer.apply_boundary / implicit_project / implicit_solve / step_slotted.  alpha is kept in float32."""

    def __init__(self, pol, step_dt):
        self.pol = pol
        self.fields = []        # [(level set, its speed bound)]
        self.alpha = np.float32(0)
        self.stats = None
        self.set_step_dt(step_dt)

    def set_step_dt(self, step_dt):
        if not (np.isfinite(step_dt) and step_dt >= 0):
            raise ValueError("step_dt: finite and not negative")
        self.step_dt = float(np.float32(step_dt))

    def __len__(self):
        return len(self.fields)

    @staticmethod
    def speed_bound(ls):
        """max |v_d| a sample of ls can return: its cells and its background; 0 without a "v" property"""
        return max(ls.max_speed(), abs(float(np.float32(ls.background)))) if ls.has_velocity else 0.0

    def push(self, ls, allow_wide=False):
        """append a keyframe.  A sample point moves by up to step_dt * speed before a level set is asked: beyond that level set's band
        its stencil may be constant, the blended distance can then be negative where neither keyframe is, and the normal is 0 / 0 (as in
        the reference), so this raises ValueError when step_dt * speed exceeds the band; allow_wide=True takes the keyframe anyway.  A
        level set that does not know its band (built from keys and cells directly) is not checked."""
        speed = self.speed_bound(ls)
        band = getattr(ls, "band", None)
        if not allow_wide and band is not None and self.step_dt * speed > band:
            raise ValueError("push: step_dt * max speed = %g exceeds the level set's band %g (allow_wide=True overrides)"
                             % (self.step_dt * speed, band))
        self.fields.append((ls, speed))

    def push_from_mesh(self, mesh, voxel, band, allow_wide=False, **kw):
        """push(SparseLevelSet.from_mesh(pol, mesh, voxel, band, **kw)); returns the level set"""
        ls = SparseLevelSet.from_mesh(self.pol, mesh, voxel, band, **kw)
        self.push(ls, allow_wide=allow_wide)
        return ls

    def pop(self):
        self.fields.pop(0)

    def advance(self, ratio):
        """alpha += ratio; while alpha > 1 - 128 eps: alpha -= 1 and the front keyframe (if any) is dropped -- in float32"""
        self.alpha = np.float32(self.alpha + np.float32(ratio))
        while self.alpha > POP_THRESHOLD:
            self.alpha = np.float32(self.alpha - np.float32(1))
            if self.fields:
                self.pop()

    def enable_stats(self):
        """count how the block kernels handled each grid block: read_stats()[0] culled, [1] staged, [2] direct, [3] staged with a "v" box
        read directly"""
        import torch
        self.stats = torch.zeros(4, dtype=torch.int32, device="cuda")

    def read_stats(self, reset=True):
        self.pol.syncCtx()
        s = self.stats.cpu().numpy().astype(np.int64)
        if reset:
            self.stats.zero_()
        return s

    def view(self):
        """the zs_rocm_levelset_transition of the two front keyframes (dst = src with one); the sequence keeps them alive until the next
        view().  Raises on an empty queue."""
        if not self.fields:
            raise RuntimeError("the level-set transition queue is empty")
        (src, s0), (dst, s1) = self.fields[0], self.fields[1 if len(self.fields) > 1 else 0]
        t = LevelSetTransition()
        t.src = type(src.view).from_buffer_copy(bytes(src.view))
        t.dst = type(dst.view).from_buffer_copy(bytes(dst.view))
        t.src.stats = self.stats.data_ptr() if self.stats is not None else None
        t.stepDt, t.alpha, t.maxSpeed = self.step_dt, float(self.alpha), max(s0, s1)
        self._alive = (src, dst, t)
        return t
