"""Environments the builder never makes, written by hand from a built one.

fks_environment carries three grid geometries (collision map, SDF, normals), any float
SDF, any origin isometry, any out-of-bounds value; build_complete_environment always gives
one axis-aligned geometry in all three slots, the exact EDT and +inf.  The helpers here
derive the other kind from a built environment: both the HIP path (fks_create) and the
oracle go through ``to_c()``, so both see the same struct.

``lipschitz_constants`` restates the definition of the skip proofs' two SDF constants
(fks_device.h, fks_robot.cpp analyze_sdf) in NumPy; the tests never ask the library for them.
"""
from __future__ import annotations

import ctypes

import numpy as np

from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd.environment import GridGeometry, SimulatorEnvironment


def _mat(origin) -> np.ndarray:
    return np.asarray(origin, dtype=np.float64).reshape(3, 4)


def _geometry(g: GridGeometry, origin=None, resolution=None, num_cells=None) -> GridGeometry:
    return GridGeometry(_mat(g.origin if origin is None else origin).reshape(12).copy(),
                        float(g.resolution if resolution is None else resolution),
                        tuple(int(v) for v in (g.num_cells if num_cells is None else num_cells)))


class ForeignEnvironment(SimulatorEnvironment):
    """A SimulatorEnvironment whose three grids need not coincide.  ``geometry`` is the SDF's
    (what the base class's ``nearest`` and ``resolution`` mean); ``normals_geometry`` is the grid
    of the normal CSR and ``map_geometry`` the collision map's (it sets the microstep length
    and the self-collision cell)."""

    def __init__(self, sdf_geometry, sdf, normals_geometry, normal_offsets, normal_entries, map_geometry, oob_value=np.inf):
        super().__init__(sdf_geometry, sdf, normal_offsets, normal_entries, oob_value, None)
        self.normals_geometry = normals_geometry
        self.map_geometry = map_geometry
        assert self.sdf.size == int(np.prod(sdf_geometry.num_cells))
        assert self.normal_offsets.size == int(np.prod(normals_geometry.num_cells)) + 1
        assert self.normal_entries.size == 6 * int(self.normal_offsets[-1])

    @property
    def resolution(self) -> float:
        return self.map_geometry.resolution  # GetResolution() is the collision map's

    def to_c(self):
        env = _capi.Environment()
        env.collision_map = self.map_geometry.to_c()
        env.sdf = self.geometry.to_c()
        env.normals = self.normals_geometry.to_c()
        env.sdf_values = _capi.as_ptr(self.sdf, ctypes.c_float)
        env.sdf_oob_value = self.oob_value
        env.normal_offsets = _capi.as_ptr(self.normal_offsets, ctypes.c_uint32)
        env.normal_entries = _capi.as_ptr(self.normal_entries, ctypes.c_double) if self.normal_entries.size else None
        return env, [self.sdf, self.normal_offsets, self.normal_entries]

    def grid_coordinates(self, points: np.ndarray) -> np.ndarray:
        """(n,3) world points in SDF cells (inverse origin isometry, then / resolution)."""
        o = _mat(self.geometry.origin)
        return ((np.asarray(points, dtype=np.float64)[:, :3] - o[:, 3]) @ o[:, :3]) * (1.0 / self.geometry.resolution)

    def nearest(self, points: np.ndarray) -> np.ndarray:
        """The nearest-cell SDF value (truncating index) under any origin isometry."""
        g = self.grid_coordinates(points)
        idx = np.trunc(g).astype(np.int64)
        n = np.array(self.geometry.num_cells)
        ok = np.all((idx >= 0) & (idx < n), axis=1)
        out = np.full(len(g), self.oob_value, dtype=np.float64)
        lin = (idx[ok, 0] * n[1] + idx[ok, 1]) * n[2] + idx[ok, 2]
        out[ok] = self.sdf[lin]
        return out

    def replaced(self, **kw) -> "ForeignEnvironment":
        a = dict(sdf_geometry=self.geometry, sdf=self.sdf, normals_geometry=self.normals_geometry,
                 normal_offsets=self.normal_offsets, normal_entries=self.normal_entries, map_geometry=self.map_geometry,
                 oob_value=self.oob_value)
        a.update(kw)
        return ForeignEnvironment(**a)


def foreign(env: SimulatorEnvironment) -> ForeignEnvironment:
    """The built environment as it is (one geometry in the three slots), ready to be changed."""
    if isinstance(env, ForeignEnvironment):
        return env
    g = env.geometry
    return ForeignEnvironment(_geometry(g), env.sdf.copy(), _geometry(g), env.normal_offsets.copy(), env.normal_entries.copy(),
                              _geometry(g), env.oob_value)


def lipschitz_constants(sdf: np.ndarray, num_cells, resolution: float):
    """(lplus, cmax) in cells, or None when a value is not finite (skipping is then off):
    over axis-neighbour pairs, lplus = max |a - b| / res where both are positive, cmax =
    max a / res over positive cells with a non-positive neighbour."""
    v = np.asarray(sdf, dtype=np.float64).reshape(tuple(num_cells))
    if not np.all(np.isfinite(v)):
        return None
    lplus = cmax = 0.0
    for axis in range(3):
        a = np.moveaxis(v, axis, 0)[:-1]
        b = np.moveaxis(v, axis, 0)[1:]
        both = (a > 0.0) & (b > 0.0)
        if both.any():
            lplus = max(lplus, float(np.max(np.abs(a - b)[both])))
        for p, q in ((a, b), (b, a)):
            edge = (p > 0.0) & ~(q > 0.0)
            if edge.any():
                cmax = max(cmax, float(np.max(p[edge])))
    return lplus / resolution, cmax / resolution


# ---------------------------------------------------------------- isometries
def isometry(R, t) -> np.ndarray:
    T = np.zeros((3, 4))
    T[:, :3] = np.asarray(R, dtype=np.float64)
    T[:, 3] = np.asarray(t, dtype=np.float64)
    return T


def compose(A, B) -> np.ndarray:
    """A * B for 3x4 isometries."""
    A, B = _mat(A), _mat(B)
    out = np.zeros((3, 4))
    out[:, :3] = A[:, :3] @ B[:, :3]
    out[:, 3] = A[:, :3] @ B[:, 3] + A[:, 3]
    return out


def rotated(env, R, t) -> ForeignEnvironment:
    """The same cell data declared under the origin T * origin (T = (R | t)) in all three
    slots; both 3-vectors of every 6-double normal entry are rotated by R."""
    e = foreign(env)
    T = isometry(R, t)
    ent = e.normal_entries.reshape(-1, 2, 3) @ np.asarray(R, dtype=np.float64).T
    return e.replaced(sdf_geometry=_geometry(e.geometry, origin=compose(T, e.geometry.origin)),
                      normals_geometry=_geometry(e.normals_geometry, origin=compose(T, e.normals_geometry.origin)),
                      map_geometry=_geometry(e.map_geometry, origin=compose(T, e.map_geometry.origin)),
                      normal_entries=np.ascontiguousarray(ent.reshape(-1)))


# ---------------------------------------------------------------- other SDFs
def scaled(env, s: float) -> ForeignEnvironment:
    e = foreign(env)
    return e.replaced(sdf=(e.sdf * np.float32(s)).astype(np.float32))


def cliff(env, at_cells: float, jump_cells: float) -> ForeignEnvironment:
    """Every value above at_cells * res raised by jump_cells * res: lplus ~ jump + 1, and no
    value near a surface changes."""
    e = foreign(env)
    res = np.float32(e.geometry.resolution)
    sdf = np.where(e.sdf > np.float32(at_cells) * res, e.sdf + np.float32(jump_cells) * res, e.sdf).astype(np.float32)
    return e.replaced(sdf=sdf)


def pit(env, cell, z_range, value_cells: float = -2.0) -> ForeignEnvironment:
    """A short column of isolated negative cells at (cell[0], cell[1], z_range) in open space;
    its neighbours keep their positive values, so cmax becomes the largest of them."""
    e = foreign(env)
    sdf = e.sdf.reshape(e.geometry.num_cells).copy()
    sdf[int(cell[0]), int(cell[1]), int(z_range[0]):int(z_range[1])] = np.float32(value_cells * e.geometry.resolution)
    return e.replaced(sdf=sdf.reshape(-1))


def with_nonfinite(env, cells) -> ForeignEnvironment:
    e = foreign(env)
    sdf = e.sdf.reshape(e.geometry.num_cells).copy()
    for c in cells:
        sdf[tuple(int(v) for v in c)] = np.inf
    return e.replaced(sdf=sdf.reshape(-1))


# ---------------------------------------------------------------- other grids
def _sub_origin(g: GridGeometry, lo) -> np.ndarray:
    """The origin of the sub-box of g that starts at cell lo."""
    return compose(g.origin, isometry(np.eye(3), np.asarray(lo, dtype=np.float64) * g.resolution))


def _cut_csr(offsets, entries, num_cells, lo, size):
    n = tuple(int(v) for v in num_cells)
    lin = np.arange(int(np.prod(n)), dtype=np.int64).reshape(n)
    sel = lin[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]].reshape(-1)
    counts = (offsets[sel + 1].astype(np.int64) - offsets[sel].astype(np.int64))
    new_off = np.zeros(len(sel) + 1, dtype=np.uint32)
    new_off[1:] = np.cumsum(counts)
    ent = entries.reshape(-1, 6)
    pick = np.concatenate([np.arange(offsets[c], offsets[c + 1], dtype=np.int64) for c in sel[counts > 0]]) \
        if np.any(counts > 0) else np.zeros(0, dtype=np.int64)
    return new_off, np.ascontiguousarray(ent[pick].reshape(-1))


def normals_sub_box(env, lo, size) -> ForeignEnvironment:
    """The normals on the sub-box [lo, lo + size) of the SDF grid, under its own (shifted)
    origin, the CSR cut to match: contacts outside it find no normal grid (NORMAL_OOB)."""
    e = foreign(env)
    off, ent = _cut_csr(e.normal_offsets, e.normal_entries, e.normals_geometry.num_cells, lo, size)
    g = _geometry(e.normals_geometry, origin=_sub_origin(e.normals_geometry, lo), num_cells=size)
    return e.replaced(normals_geometry=g, normal_offsets=off, normal_entries=ent)


def coarse_map(env, factor: int = 2) -> ForeignEnvironment:
    """A collision map at `factor` times the SDF's cell size over the same box."""
    e = foreign(env)
    g = e.map_geometry
    return e.replaced(map_geometry=_geometry(g, resolution=g.resolution * factor,
                                             num_cells=[max(2, -(-int(v) // factor)) for v in g.num_cells]))


def cropped(env, lo, size) -> ForeignEnvironment:
    """All three grids cut to the sub-box [lo, lo + size) of a built scene (cell counts that
    are no multiple of the 4-cell brick, for instance)."""
    e = foreign(env)
    n = e.geometry.num_cells
    sdf = e.sdf.reshape(n)[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]]
    off, ent = _cut_csr(e.normal_offsets, e.normal_entries, e.normals_geometry.num_cells, lo, size)
    o = _sub_origin(e.geometry, lo)
    return e.replaced(sdf_geometry=_geometry(e.geometry, origin=o, num_cells=size), sdf=np.ascontiguousarray(sdf).reshape(-1),
                      normals_geometry=_geometry(e.normals_geometry, origin=o, num_cells=size), normal_offsets=off,
                      normal_entries=ent, map_geometry=_geometry(e.map_geometry, origin=o, num_cells=size))


def with_oob(env, value: float) -> ForeignEnvironment:
    return foreign(env).replaced(oob_value=float(value))
