"""A high-precision reference of one contact-resolver iteration, written from the definitions:
the reference simulator's header (SPCS = simple_particle_contact_simulator.hpp, cited by line) and
the documented behaviour of sdf_tools / arc_utilities / Eigen as DESIGN.md §2.2 restates it.  Not
written from oracle/ or the kernels.

It runs in the backends of tests/hp_reference.py (80-bit long double, or mpmath at 40 digits) and
reuses that module's forward kinematics, Jacobians and clean ApplyControlInput.  Inputs are the
float64 / float32 values of the environment, the robot and the recorded configurations, taken
exactly.  The only float arithmetic that is part of a definition is the float32 subtraction of the
SDF gradient: the exact difference of the two stored floats is rounded to float32 once.

What is stated here:

* grid cell = trunc((inv_origin . p) / res) per axis with a bounds test; SDF value of that cell;
  gradient = central differences of the stored floats (one-sided at the faces); EstimateDistance4d
  = nominal value moved res/2 toward zero + gradient . (p - cell centre), a sign flip against the
  nominal value replaced by +-res/16, (oob, false) outside;
* CheckEnvironmentCollision (SPCS:921-981): threshold t - tolerance res; the nearest value first,
  the estimate only inside the one-cell band;
* the surface-normal lookup (SPCS:111-132, 186-256): largest dot product of entry direction and unit
  motion, strict >, first wins, an empty cell gives a zero normal;
* CollectSelfCollisions / ExtractSelfCollidingPoints (SPCS:983-1275): extended keys trunc(g / res),
  suffix-sum masses, per-link momenta, C, N, M, V, impulses = (N'C'M^-1 C N)^-1 N'C'V, correction
  = -(M^-1 C N impulses)[0:3] / points of the link in the cell; CheckSelfCollisions (SPCS:1277-1396);
* CollectPointCorrectionsAndJacobians (SPCS:1818-1939);
* the stacked and the individual-Jacobian least-squares steps (SPCS:1966-1998): the basic solution
  of a column-pivoted Householder QR, pivot = largest residual squared column norm (an exact tie
  goes to the lower index), stop at Eigen's threshold maxColSqNorm eps^2 / R (R - k), eps of float64;
* EstimateMaxControlInputWorkspaceMotion (SPCS:1492-1544), step_fraction = max(motion / res, 1), the
  scaling schedule of SPCS:1624 and 1747-1761, the microstep count of SPCS:1551-1568 and
  CheckConfigCollision (SPCS:1398-1416).

Every discrete decision records its margin (class Margins).  A decision is *near* when its
deciding quantity lies within NEAR = 1e-9 of its threshold (metres for distances, absolute for dot
products and for a wrapped angle's distance to the cut, relative for pivot norms), when a grid
coordinate lies within 1e-9 cells of an integer and the neighbouring cell decides differently, or
when two unequal pivot candidates agree to 1e-9 relative and taking the rival leads to another set
of pivot columns (the order of the pivots does not change the basic solution, the set does; the
rivals' steps are returned so that a record can be held to either).  A *near rank* decision is a
pivot (or the largest residual column norm of J rounded to float64 at the structural rank: the noise
pivot of DESIGN.md §3) within a factor 1e4 of the rank threshold, either way.  An all-zero J has a
zero threshold, which the strict < never meets: its basic solution is 0 / 0 and counts as near.

Extended self-collision keys have a second reading (ContactReference.double_keys): the header
computes them in double arithmetic from the double point (SPCS:1176-1179), and static links whose
points lie on cell faces (a cylinder of radius 0.05 in a 0.01 grid) make the exact-arithmetic key
undecidable in most iterations of the self-contact scenes.  With double_keys a key within 1e-9 of an
integer is the truncated double quotient of the point rounded to double once."""
import itertools

import numpy as np

import hp_reference as H
from fast_kinematic_simulator_amd import _capi

NEAR = 1e-9
RANK_WINDOW = 1e4
EPS64 = 2.0 ** -52


class Margins:
    """The discrete decisions of one evaluation: (kind, margin) pairs, the near ones and the near
    rank decisions."""

    def __init__(self):
        self.items = []
        self.near = []
        self.near_rank = []

    def add(self, kind, margin, near=None):
        margin = float(margin)
        self.items.append((kind, margin))
        if (margin < NEAR) if near is None else near:
            self.near.append((kind, margin))

    def add_rank(self, kind, ratio):
        self.items.append((kind, float(ratio)))
        if 1.0 / RANK_WINDOW < ratio < RANK_WINDOW:
            self.near_rank.append((kind, float(ratio)))


class State:
    """A configuration with its kinematics: per-geometry transforms and world points."""

    def __init__(self, robot, q, B):
        self.q = q
        self.T = None
        if robot.robot_type == _capi.ROBOT_SE2:
            self.geometry_T = [H.se2_transform(q, B)]
        elif robot.robot_type == _capi.ROBOT_SE3:
            self.geometry_T = [H.from34(q, B)]
        else:
            self.T = H.link_transforms(robot, q, B)
            self.geometry_T = [self.T[link] for link in robot.geometry_link]
        self.points = [(B.array(p) @ T.T)[:, :3] for p, T in zip(robot.geometry_points, self.geometry_T)]
        self.all_points = np.concatenate(self.points, axis=0)


def _unit(v, B):
    """EigenHelpers::SafeNormal: v / |v| when the norm exceeds float64's epsilon, else v"""
    n = H.norm(v, B)
    return v / n if float(n) > EPS64 else v


def _solve(A, rhs, B):
    """A^-1 rhs by Gauss-Jordan elimination with partial pivoting, in the backend's arithmetic."""
    n = A.shape[0]
    M = np.concatenate([A.copy(), rhs.reshape(n, 1).copy()], axis=1)
    for c in range(n):
        p = c + int(np.argmax([abs(float(M[r, c])) for r in range(c, n)]))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n]


class Grid:
    """The voxel grid shared by the SDF, the surface normals and the collision map."""

    def __init__(self, env, B):
        g = env.geometry
        o = np.asarray(g.origin, dtype=np.float64).reshape(3, 4)
        self.B = B
        self.R, self.t = B.array(o[:, :3]), B.array(o[:, 3])
        self.res = B.scalar(float(g.resolution))
        self.res_f = float(g.resolution)
        self.n = np.array([int(v) for v in g.num_cells], dtype=np.int64)
        self.stride = np.array([self.n[1] * self.n[2], self.n[2], 1], dtype=np.int64)
        self.sdf = env.sdf.reshape(-1)
        self.oob = float(env.oob_value)
        self.offsets = env.normal_offsets
        self.entries = env.normal_entries.reshape(-1, 6)

    def coordinates(self, p, res=None):
        """(inv_origin . p) / res per axis: the origin is a rigid transform, its inverse R' (p - t)"""
        return ((p - self.t) @ self.R) / (self.res if res is None else res)

    @staticmethod
    def cells(coordinates):
        """(cell indices by truncation, per coordinate the alternative index if the coordinate lies
        within NEAR of an integer that truncation distinguishes, else the same index)"""
        cf = H.to_float(coordinates)
        idx = np.trunc(cf).astype(np.int64)
        r = np.rint(cf)
        close = (np.abs(cf - r) < NEAR) & (r != 0)
        below = np.trunc(r - np.sign(r) * 0.5).astype(np.int64)  # the cell on the side of zero
        ri = r.astype(np.int64)
        alt = np.where(close, np.where(idx == ri, below, ri), idx)
        return idx, alt

    def in_bounds(self, idx):
        return np.all((idx >= 0) & (idx < self.n), axis=1)

    def nearest(self, idx):
        """stored value of each cell as float64 (exact), the oob value outside"""
        ok = self.in_bounds(idx)
        out = np.full(len(idx), self.oob, dtype=np.float64)
        out[ok] = self.sdf[idx[ok] @ self.stride].astype(np.float64)
        return out, ok

    def estimate(self, p, idx):
        """EstimateDistance4d for in-bounds cells idx of points p: (estimate, estimate before the
        sign-flip replacement), backend arrays."""
        B = self.B
        lin = idx @ self.stride
        nominal = self.sdf[lin].astype(np.float64)
        centre = ((B.array(idx) + B.scalar(0.5)) * self.res) @ self.R.T + self.t
        d = p - centre
        raw = B.array(nominal) + np.where(nominal >= 0.0, -1.0, 1.0) * (self.res / 2)
        for a in range(3):
            i = idx[:, a]
            lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, self.n[a] - 1)
            f_hi = self.sdf[lin + (hi - i) * self.stride[a]].astype(np.float64)
            f_lo = self.sdf[lin + (lo - i) * self.stride[a]].astype(np.float64)
            diff = (f_hi - f_lo).astype(np.float32).astype(np.float64)  # float64 holds the exact difference of two floats
            span = np.maximum(hi - lo, 1)
            raw = raw + (B.array(diff) / (self.res * B.array(span))) * d[:, a]
        est = raw.copy()
        sixteenth = self.res / 16
        for k in range(len(est)):
            if nominal[k] >= 0.0 and raw[k] < 0:
                est[k] = sixteenth
            elif nominal[k] < 0.0 and raw[k] > 0:
                est[k] = -sixteenth
        return est, raw

    def alternatives(self, idx_row, alt_row):
        """the other cells a point with near-integer coordinates could fall into"""
        axes = [a for a in range(3) if alt_row[a] != idx_row[a]]
        out = []
        for choice in itertools.product([False, True], repeat=len(axes)):
            if not any(choice):
                continue
            c = idx_row.copy()
            for a, take in zip(axes, choice):
                if take:
                    c[a] = alt_row[a]
            out.append(c)
        return out


class ContactReference:
    """The resolver of one (environment, robot, solver, controller interval)."""

    def __init__(self, env, robot, solver, controller_interval, individual_jacobians=False, B=H.DEFAULT):
        self.env, self.robot, self.solver, self.B = env, robot, solver, B
        self.dt = B.scalar(float(controller_interval))
        self.individual = bool(individual_jacobians)
        self.grid = Grid(env, B)
        self.allowed = set()
        for a, b in robot.allowed_pairs:
            self.allowed.add((int(a), int(b)))
            self.allowed.add((int(b), int(a)))
        self.counts = [len(p) for p in robot.geometry_points]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)])
        self.geometry_of = np.repeat(np.arange(len(self.counts)), self.counts)
        self.point_of = np.concatenate([np.arange(c) for c in self.counts])
        self.wrapped = self._wrapped_elements()
        self.self_info = {}  # (geometry, point) -> scales of its correction in the last self-collision map
        self.double_keys = False  # see _self_keys

    # ------------------------------------------------------------ configurations
    def state(self, q):
        return State(self.robot, q, self.B)

    def set_position(self, q):
        """SetPosition: the limits and wraps of a clean ApplyControlInput of zero"""
        return H.apply_control_input(self.robot, q, np.zeros(self.robot.num_dofs), self.B)

    def apply(self, q, u):
        return H.apply_control_input(self.robot, q, u, self.B)

    def _wrapped_elements(self):
        if self.robot.robot_type == _capi.ROBOT_SE2:
            return [2]
        if self.robot.robot_type == _capi.ROBOT_SE3:
            return []
        moving = [j for j in self.robot.joints if j.type != _capi.JOINT_FIXED]
        return [k for k, j in enumerate(moving) if j.type == _capi.JOINT_CONTINUOUS]

    def self_collision_allowed(self, a, b):
        return a == b or (a, b) in self.allowed

    def max_motion(self, s0, s1):
        """EstimateMaxControlInputWorkspaceMotion (SPCS:1492-1527): the largest point displacement"""
        d = s1.all_points - s0.all_points
        sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        return self.B.sqrt(max(sq))

    # ------------------------------------------------------------ environment
    def environment_collision(self, st, threshold, M):
        """CheckEnvironmentCollision (SPCS:921-981) with collision_threshold `threshold`.  The first hit
        ends the reference's loop; the verdict is "any point hits", so every point is evaluated here and
        the verdict is near only if no hit is clear (or, when free, if any point is near)."""
        B, G = self.B, self.grid
        thr = B.scalar(threshold) - B.scalar(float(self.solver.environment_collision_check_tolerance)) * G.res
        idx, alt = G.cells(G.coordinates(st.all_points))
        hit, margin = self._environment_hits(st.all_points, idx, thr)
        for k in np.nonzero(np.any(alt != idx, axis=1))[0]:
            for c in G.alternatives(idx[k], alt[k]):
                h, _ = self._environment_hits(st.all_points[k:k + 1], c[None, :], thr)
                if h[0] != hit[k]:
                    margin[k] = 0.0
        verdict = bool(np.any(hit))
        if verdict:
            M.add("environment check", float(np.max(margin[hit])))
        else:
            M.add("environment check", float(np.min(margin)))
        return verdict

    def _environment_hits(self, p, idx, thr):
        G = self.grid
        thr_f = float(thr)
        nominal, ok = G.nearest(idx)
        cand = ok & (nominal < thr_f)
        deep = cand & (nominal < thr_f - G.res_f)
        margin = np.abs(nominal - thr_f)
        margin[cand] = np.minimum(margin[cand], np.abs(nominal[cand] - (thr_f - G.res_f)))
        hit = deep.copy()
        band = np.nonzero(cand & ~deep)[0]
        if len(band):
            est, raw = G.estimate(p[band], idx[band])
            for k, e, r in zip(band, est, raw):
                hit[k] = bool(e < thr)
                margin[k] = min(margin[k], abs(float(e - thr)))
                if abs(float(r)) < NEAR and bool(r < thr) != bool(G.res / 16 * (1 if nominal[k] >= 0 else -1) < thr):
                    margin[k] = 0.0
        return hit, margin

    # ------------------------------------------------------------ self collisions
    def _cells_of(self, keys):
        cells = {}
        for k, key in enumerate(map(tuple, keys.tolist())):
            cells.setdefault(key, []).append(k)
        return cells

    def _self_keys(self, st, resolution):
        """Extended-cell keys and their alternatives.  With double_keys set, a key within NEAR of an
        integer is taken as the header states it, in double arithmetic (SPCS:1176-1179: the point in the
        grid frame is a double vector, the key the truncated double quotient), from the point rounded to
        double once; it then has no alternative.  The grid origins here are pure translations, so the
        grid-frame point costs the one rounding of p - t."""
        G = self.grid
        keys, alt = Grid.cells(G.coordinates(st.all_points, resolution))
        if self.double_keys:
            t, R = H.to_float(G.t), H.to_float(G.R)
            assert np.array_equal(R, np.eye(3)), "double keys are stated for translated grids only"
            keys64 = np.trunc((H.to_float(st.all_points) - t) / float(resolution)).astype(np.int64)
            keys = np.where(alt != keys, keys64, keys)
            alt = keys
        return keys, alt

    def _cell_links(self, members):
        """per geometry with a point in the cell, its points (ascending geometry: a std::map)"""
        by = {}
        for k in members:
            by.setdefault(int(self.geometry_of[k]), []).append(int(self.point_of[k]))
        return dict(sorted(by.items()))

    def _no_self_collisions(self):
        n = len(self.counts)
        return n == 1 or (n == 2 and self.self_collision_allowed(0, 1))

    def _masses(self):
        masses, total = {}, 0
        for g in range(len(self.counts) - 1, -1, -1):  # SPCS:1243-1255: a link's mass includes every further link's
            total += self.counts[g]
            masses[g] = total
        return masses

    def _cell_corrections(self, members, prev, cur):
        """ExtractSelfCollidingPoints (SPCS:983-1171) for the points `members` (flat indices, in geometry-
        then-point order) of one extended cell: {(geometry, point): correction}"""
        B = self.B
        out = {}
        if len(members) < 2:
            return out
        by = self._cell_links(members)
        if len(by) < 2:
            return out
        coll = {f: [s for s in by if s != f and not self.self_collision_allowed(f, s)] for f in by}
        coll = {f: o for f, o in coll.items() if o}
        if len(coll) < 2:
            return out
        masses = self._masses()
        momentum = {}
        for f in coll:
            m = B.zeros(3)
            for i in by[f]:
                m = m + (cur.points[f][i] - prev.points[f][i]) / self.dt
            momentum[f] = m
        for f, others in coll.items():
            n = len(others)
            p0 = prev.points[f][by[f][0]]
            C, N = B.zeros((3 * (n + 1), 3 * n)), B.zeros((3 * n, n))
            Minv, V = B.zeros((3 * (n + 1), 3 * (n + 1))), B.zeros(3 * (n + 1))
            Minv[:3, :3] = B.eye(3) / B.scalar(masses[f])
            V[:3] = momentum[f] / B.scalar(len(by[f]))
            for k, o in enumerate(others):
                C[0:3, 3 * k:3 * k + 3] = -B.eye(3)
                C[3 * (k + 1):3 * (k + 2), 3 * k:3 * k + 3] = B.eye(3)
                N[3 * k:3 * k + 3, k] = _unit(prev.points[o][by[o][0]] - p0, B)
                Minv[3 * (k + 1):3 * (k + 2), 3 * (k + 1):3 * (k + 2)] = B.eye(3) / B.scalar(masses[o])
                V[3 * (k + 1):3 * (k + 2)] = momentum[o] / B.scalar(len(by[o]))
            CN = C @ N
            A = CN.T @ Minv @ CN
            impulses = _solve(A, CN.T @ V, B)
            delta = -(Minv @ CN @ impulses)
            # what a tolerance on this correction scales with: the fastest link, the shortest normal
            # baseline, the conditioning of the impulse matrix, the links involved
            speeds = [float(H.norm(V[3 * k:3 * k + 3], B)) for k in range(n + 1)]
            spans = [float(H.norm(prev.points[o][by[o][0]] - p0, B)) for o in others]
            info = (max(speeds), min(spans), float(np.linalg.cond(H.to_float(A))), n + 1)
            for i in by[f]:
                out[(f, i)] = (delta[:3] / B.scalar(len(by[f])), info)
        return out

    def _cell_collides(self, members):
        """CheckPointsForSelfCollision (SPCS:1277-1322): two links in the cell that may not touch"""
        if len(members) < 2:
            return False
        by = self._cell_links(members)
        return any(not self.self_collision_allowed(f, s) for f in by for s in by if f != s)

    def _same_outcome(self, a, b):
        if isinstance(a, bool):
            return a == b
        return a.keys() == b.keys() and all(H.max_abs_diff(a[k][0], H.to_float(b[k][0]), self.B) < NEAR for k in a)

    def _key_margins(self, keys, alt, cells, outcome, M):
        """A key coordinate within NEAR of an integer is near if the other cell changes the outcome.
        Moving one point changes two cells only: the one it leaves and the one it joins."""
        worst = np.inf
        for k in np.nonzero(np.any(alt != keys, axis=1))[0]:
            k = int(k)
            home = cells[tuple(int(v) for v in keys[k])]
            for c in self.grid.alternatives(keys[k], alt[k]):
                there = cells.get(tuple(int(v) for v in c), [])
                geometries = {int(self.geometry_of[m]) for m in home} | {int(self.geometry_of[m]) for m in there}
                if len(geometries) < 2:
                    continue  # one link alone decides nothing, wherever its points fall
                left, joined = [m for m in home if m != k], sorted(there + [k])
                if not (self._same_outcome(outcome(home), outcome(left)) and self._same_outcome(outcome(there), outcome(joined))):
                    worst = 0.0
        M.add("self-collision cell", worst)

    def self_collisions(self, prev, cur, M):
        """CollectSelfCollisions (SPCS:1183-1275): {(geometry, point): correction}"""
        out = {}
        self.self_info = {}
        if self._no_self_collisions():
            return out
        keys, alt = self._self_keys(cur, self.grid.res)
        cells = self._cells_of(keys)
        for members in cells.values():
            for key, (correction, info) in self._cell_corrections(members, prev, cur).items():
                out[key] = correction
                self.self_info[key] = info
        self._key_margins(keys, alt, cells, lambda members: self._cell_corrections(members, prev, cur), M)
        return out

    def self_check(self, st, resolution, M):
        """CheckSelfCollisions (SPCS:1324-1396) at `resolution`"""
        if self._no_self_collisions():
            return False
        keys, alt = self._self_keys(st, resolution)
        cells = self._cells_of(keys)
        self._key_margins(keys, alt, cells, self._cell_collides, M)
        return any(self._cell_collides(members) for members in cells.values())

    # ------------------------------------------------------------ collision verdicts
    def in_collision(self, prev, cur, M, self_map=None):
        """CheckCollision (SPCS:1418-1436): (verdict, self-collision map)"""
        env = self.environment_collision(cur, 0.0, M)
        if self_map is None:
            self_map = self.self_collisions(prev, cur, M)
        return env or len(self_map) > 0, self_map

    def check_config_collision(self, q, inflation_ratio):
        """CheckConfigCollision (SPCS:1398-1416): (verdict, margins)"""
        B, M = self.B, Margins()
        st = self.state(self.set_position(q))
        env = self.environment_collision(st, B.scalar(float(inflation_ratio)) * self.grid.res, M)
        own = self.self_check(st, (B.scalar(float(inflation_ratio)) + 1) * self.grid.res, M)
        M.parts = (env, own)  # which of the two checks decided
        return env or own, M

    def shallowest_penetration(self, q):
        """The largest EstimateDistance4d value before the sign-flip replacement among the points of
        configuration q in cells of negative distance (+inf when there is none), as a float.  Stored
        distances are multiples of the cell size, so the environment check depends on a threshold of a
        fraction of a cell only through these estimates; tests use this to place configurations."""
        G = self.grid
        st = self.state(self.set_position(q))
        idx, _ = G.cells(G.coordinates(st.all_points))
        nominal, ok = G.nearest(idx)
        inside = ok & (nominal < 0.0)
        if not np.any(inside):
            return np.inf
        _, raw = G.estimate(st.all_points[inside], idx[inside])
        return max(float(v) for v in raw)

    def microsteps(self, q, real_control_input):
        """SPCS:1559-1562: max(1, ceil(motion(u dt) / (res / 8))); (count, margins)"""
        M = Margins()
        s0 = self.state(q)
        s1 = self.state(self.apply(q, real_control_input))
        x = float(self.max_motion(s0, s1) / (self.grid.res / 8))
        M.add("microstep count", abs(x - np.rint(x)))
        return max(1, int(np.ceil(x))), M

    # ------------------------------------------------------------ corrections
    def jacobian(self, st, g, i):
        p = np.asarray(self.robot.geometry_points[g][i], dtype=np.float64)
        if self.robot.robot_type == _capi.ROBOT_SE2:
            return H.se2_jacobian(st.q, p, self.B)
        if self.robot.robot_type == _capi.ROBOT_SE3:
            return H.se3_jacobian(st.q, p, self.B)
        return H.point_jacobian(self.robot, st.q, g, p, self.B, T=st.T)

    def _environment_correction(self, p, motion, cell, M=None):
        """(corrected, correction) of a point at p in `cell` (SPCS:1863-1891)"""
        B, G = self.B, self.grid
        nominal, ok = G.nearest(cell[None, :])
        if not ok[0] or nominal[0] >= 0.0:
            return False, None  # an estimate below 0 needs a negative nominal value: the flip rule gives +res/16 otherwise
        est, raw = G.estimate(p[None, :], cell[None, :])
        if M is not None:
            M.add("estimate sign", abs(float(raw[0])))
        if not est[0] < 0:
            return False, None
        lin = int(cell @ G.stride)
        entries = G.entries[int(G.offsets[lin]):int(G.offsets[lin + 1])]
        normal = B.zeros(3)
        if len(entries):
            unit = _unit(motion, B)
            dots = [e[0] * unit[0] + e[1] * unit[1] + e[2] * unit[2] for e in B.array(entries[:, :3])]
            best = 0
            for k in range(1, len(dots)):
                if dots[k] > dots[best]:
                    best = k
            if M is not None:
                # an exact tie is decided by the rule (strict >: the first wins); unequal products within NEAR
                # of the largest are near if their normals differ
                rivals = [float(dots[best] - dots[k]) for k in range(len(dots))
                          if dots[k] != dots[best] and not np.array_equal(entries[k, 3:], entries[best, 3:])]
                M.add("normal choice", min(rivals, default=np.inf))
            normal = _unit(B.array(entries[best, 3:]), B)
        return True, normal * abs(est[0])

    def corrections(self, prev, cur, self_map, M):
        """CollectPointCorrectionsAndJacobians (SPCS:1818-1939): (J, b, the corrected (geometry, point)s)"""
        B, G = self.B, self.grid
        idx, alt = G.cells(G.coordinates(cur.all_points))
        nominal, ok = G.nearest(idx)
        rows_J, rows_b, who = [], [], []
        flat = 0
        for g, count in enumerate(self.counts):
            for i in range(count):
                k = flat
                flat += 1
                own = self_map.get((g, i))
                near_cell = bool(np.any(alt[k] != idx[k]))
                if own is None and not near_cell and not (ok[k] and nominal[k] < 0.0):
                    continue
                motion = cur.all_points[k] - prev.all_points[k]
                has, env = self._environment_correction(cur.all_points[k], motion, idx[k], M)
                if near_cell:
                    for c in G.alternatives(idx[k], alt[k]):
                        has2, env2 = self._environment_correction(cur.all_points[k], motion, c)
                        if has2 != has or (has and H.max_abs_diff(env2, H.to_float(env), B) > NEAR):
                            M.add("correction cell", 0.0)
                if own is None and not has:
                    continue
                b = B.zeros(3)
                if own is not None:
                    b = b + own
                if has:
                    b = b + env
                rows_J.append(self.jacobian(cur, g, i))
                rows_b.append(b)
                who.append((g, i))
        D = self.robot.num_dofs
        if not who:
            return B.zeros((0, D)), B.zeros(0), who
        return np.concatenate(rows_J, axis=0), np.concatenate(rows_b, axis=0), who

    # ------------------------------------------------------------ least squares
    def colpiv_qr(self, J, b, M=None, steps=None, force=None, ties=None):
        """Basic solution of column-pivoted Householder QR (SPCS:1994, Eigen's ColPivHouseholderQR).
        steps: factor exactly that many columns whatever the threshold says.  force: {step: column} to
        take at those steps instead of the largest.  ties: a list that receives (step, rival column) for
        every unequal candidate within NEAR (relative, of the norms) of the pivot taken.  Returns (x,
        pivot columns in order, ratio of the largest residual column norm to the rank threshold where it
        stopped)."""
        B = self.B
        A, c = J.copy(), b.copy()
        R, D = A.shape
        size = min(R, D)
        perm = list(range(D))
        sq0 = list((A * A).sum(axis=0))
        helper = max(sq0) * B.scalar(EPS64) * B.scalar(EPS64) / R
        rank, stop_ratio = 0, None
        if M is not None:
            # an all-zero J (points of a link no dof moves): threshold and pivot are both zero, the strict <
            # does not stop and the basic solution is 0 / 0 -- nothing to compare a record with
            M.add("zero system", np.inf if float(max(sq0)) > 0 else 0.0)
        for k in range(size):
            sq = list((A[k:, k:] * A[k:, k:]).sum(axis=0))
            best = 0
            for j in range(1, len(sq)):
                if sq[j] > sq[best]:
                    best = j
            threshold = helper * (R - k)
            ratio = float(B.sqrt(sq[best] / threshold)) if float(threshold) > 0 else (np.inf if float(sq[best]) > 0 else 0.0)
            if steps is None:
                if M is not None:
                    M.add_rank("rank threshold", ratio)
                if sq[best] < threshold or float(sq[best]) == 0.0:
                    stop_ratio = ratio
                    break
                if ties is not None:
                    ties += [(k, perm[k + j]) for j, v in enumerate(sq)
                             if v != sq[best] and abs(float((sq[best] - v) / sq[best])) < 2 * NEAR]
                if force is not None and k in force:
                    best = perm.index(force[k]) - k
            elif k == steps:
                stop_ratio = ratio
                break
            if best:
                A[:, [k, k + best]] = A[:, [k + best, k]]
                perm[k], perm[k + best] = perm[k + best], perm[k]
            x = A[k:, k].copy()
            tail = sum(v * v for v in x[1:]) if len(x) > 1 else B.scalar(0.0)
            if float(tail) != 0.0:
                beta = B.sqrt(x[0] * x[0] + tail)
                if x[0] >= 0:
                    beta = -beta
                v = x / (x[0] - beta)
                v[0] = B.scalar(1.0)
                tau = (beta - x[0]) / beta
                w = v @ A[k:, k:]
                A[k:, k:] = A[k:, k:] - tau * np.outer(v, w)
                c[k:] = c[k:] - tau * v * (v @ c[k:])
            rank = k + 1
        y = [None] * rank
        for i in range(rank - 1, -1, -1):
            s = c[i]
            for j in range(i + 1, rank):
                s = s - A[i, j] * y[j]
            y[i] = s / A[i, i]
        out = B.zeros(D)
        for i in range(rank):
            out[perm[i]] = y[i]
        return out, perm[:rank], stop_ratio

    def _solve_block(self, J, b, M):
        """one least-squares solve with its rank margins: (x, pivot columns, kappa_2 of the pivot columns)"""
        ties = []
        x, S, _ = self.colpiv_qr(J, b, M, ties=ties)
        # two unequal candidates within NEAR: the order of the pivots does not matter to the basic solution,
        # the set of pivot columns does (the least-squares solution on full-rank columns is unique), so
        # the tie is a near decision when taking the rival leads to another set
        rivals, queue, runs = {}, [{k: c} for k, c in ties], 0
        while queue and runs < 16:  # ties within a rival's own factorisation are followed too, up to 16 factorisations
            force = queue.pop(0)
            runs += 1
            more = []
            xa, Sa, _ = self.colpiv_qr(J, b, force=force, ties=more)
            if set(Sa) != set(S):
                rivals.setdefault(frozenset(Sa), (xa, Sa))
            queue += [{**force, k: c} for k, c in more if k > max(force)]
        M.add("pivot choice", 0.0 if rivals else np.inf)
        if len(S) < min(J.shape):
            # the noise pivot: what is left of J rounded to float64 once the structural rank is factored
            J64 = self.B.array(H.to_float(J))
            _, _, ratio = self.colpiv_qr(J64, b, None, steps=len(S))
            if ratio is not None:
                M.add_rank("noise pivot", ratio)
        Jf = H.to_float(J)

        def kappa(columns):
            if not columns:
                return 1.0
            sv = np.linalg.svd(Jf[:, columns], compute_uv=False)
            return float(sv[0] / sv[-1])

        return x, S, kappa(S), [(xa, Sa, kappa(Sa)) for xa, Sa in rivals.values()]

    def correction_step(self, J, b, M):
        """SPCS:1629: the stacked solve, or the sum of the per-point solves (SPCS:1966-1988).  Returns
        (raw step, [(rows, pivot columns, kappa)] per solve, [(raw step, solves)] of the stacked solve's
        near pivot ties that lead to another set of pivot columns: one tie each)."""
        if not self.individual:
            x, S, kappa, rivals = self._solve_block(J, b, M)
            return x, [(J.shape[0], S, kappa)], [(xa, [(J.shape[0], Sa, ka)]) for xa, Sa, ka in rivals]
        total, blocks = self.B.zeros(J.shape[1]), []
        for r in range(0, J.shape[0], 3):
            x, S, kappa, _ = self._solve_block(J[r:r + 3], b[r:r + 3], M)
            total = total + x
            blocks.append((3, S, kappa))
        return total, blocks, []

    def scaling(self, iteration):
        """correction_step_scaling at resolver iteration `iteration` (0-based): SPCS:1624, 1747-1761"""
        B, s = self.B, self.solver
        scale = B.scalar(float(s.resolve_correction_initial_step_size))
        floor = B.scalar(float(s.resolve_correction_min_step_scaling))
        for done in range(1, iteration + 1):
            if done % int(s.resolve_correction_step_scaling_decay_iterations) == 0:
                if scale >= 0:
                    scale = scale * B.scalar(float(s.resolve_correction_step_scaling_decay_rate))
                    if scale < floor:
                        scale = -floor
                else:
                    scale = -floor
        return scale

    # ------------------------------------------------------------ one iteration
    def iterate(self, previous, active, iteration):
        """One pass of the loop of SPCS:1625-1762 from `active` in the microstep that started at
        `previous`: a dict with the next configuration, the collision verdict after it, J, b, the
        margins and what the bound needs (the solves, the corrected points, the raw step)."""
        B, M = self.B, Margins()
        prev, cur = self.state(previous), self.state(active)
        self_map = self.self_collisions(prev, cur, M)
        self_info = dict(self.self_info)  # of this map: the verdict's check below fills it again
        J, b, who = self.corrections(prev, cur, self_map, M)
        out = {"J": J, "b": b, "corrected": who, "margins": M, "self_corrected": len(self_map), "self_info": self_info}
        if not who:
            out.update(next=None, in_collision=None, solves=[], raw_step=None, real_step=None, rivals=[])
            return out
        raw, solves, rivals = self.correction_step(J, b, M)
        out.update(self._step(prev, cur, active, iteration, raw, solves, M))
        out["rivals"] = [(raw_a, solves_a) for raw_a, solves_a in rivals]
        return out

    def rival(self, previous, active, iteration, raw, solves):
        """the rest of the iteration for the raw step of a rival pivot set (correction_step)"""
        M = Margins()
        out = self._step(self.state(previous), self.state(active), active, iteration, raw, solves, M)
        out["margins"] = M
        return out

    def _step(self, prev, cur, active, iteration, raw, solves, M):
        """SPCS:1630, 1681-1698: scale the raw step, apply it, check for collisions"""
        B = self.B
        motion = self.max_motion(cur, self.state(self.apply(active, raw)))
        fraction = max(motion / self.grid.res, B.scalar(1.0))
        real = raw / fraction * abs(self.scaling(iteration))
        nxt = self.apply(active, real)
        for k in self.wrapped:
            M.add("angle cut", float(B.pi) - abs(float(nxt[k])))
        verdict, _ = self.in_collision(prev, self.state(nxt), M)
        return dict(next=nxt, in_collision=verdict, solves=solves, raw_step=raw, real_step=real, step_fraction=float(fraction))


_CACHE = {}


def resolver_iteration(env, robot, solver, previous, active, iteration, controller_interval, individual_jacobians=False,
                       B=H.DEFAULT):
    """The resolver iteration `iteration` (0-based within its microstep) from `active`, in the microstep
    that started at `previous`: (next configuration, in-collision verdict after it, J, b, Margins)."""
    key = (id(env), id(robot), id(solver), float(controller_interval), bool(individual_jacobians), B.kind)
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = (ContactReference(env, robot, solver, controller_interval, individual_jacobians, B), env, robot, solver)
    r = _CACHE[key][0].iterate(previous, active, iteration)
    return r["next"], r["in_collision"], r["J"], r["b"], r["margins"]
