"""Root motion of a CARLA animation from its planted feet: the definition of K40 and the streaming class on top of
``ops.root_motion_carla_rows``.

Every exporter (K30, K32, K35, K36) takes the root row of a frame from ``world_loc`` / ``world_rot``, and those come from
``ZeroTrajectory``, the only trajectory model there is: a played animation swings its legs and stays on its spawn point. The
displacement is in the rows all the same: the bone that stands on the ground should not move in the world, so whatever it moves
in the actor's frame, the actor has to move the other way. The reference has nothing of the kind.

All of the following per video ``n`` and global frame ``g = first_frame + t``, in the tensor space of ``ops.carla_pose_import``
(a row (x, y, z, pitch, yaw, roll) is the location (x, y, -z) and the matrix Rx Ry Rz of radians(-roll, -pitch, -yaw)); lengths
are in the rows' unit, whatever the exporter wrote.

1. Positions. ``(l_j, R_j)`` of ``bones[n, t, j]``; ``(x_j, A_j)`` the forward kinematics over the 26-bone tree in row-vector
   form, ``x_c = l_c @ A_p + x_p``, ``A_c = R_c @ A_p`` (``data/carla/reference.forward_kinematics``); ``(r, W)`` of
   ``root[n, t]``, the actor as one more parent: ``p_k = x_{C_k} @ W + r`` for the four contact candidates ``C = (crl_foot__R,
   crl_toe__R, crl_foot__L, crl_toe__L)``; ``h_k = -p_k[2]`` is CARLA's world z of the joint. ``root=None`` means all-zero root
   rows: the actor at the origin, not rotated. An input root that already carries a trajectory is honoured: ``r`` is inside
   ``p_k``, so only what the planted joint still moves is added.
2. Step of a frame pair, ``g >= 1``: ``m_k = max(h_k(g - 1), h_k(g))``, ``s`` the smallest ``k`` with minimal ``m_k`` -- the joint
   that is lowest over BOTH frames, so a foot that has just landed or is just lifting loses to the one that stays down --
   ``d = p_s(g - 1)[0:2] - p_s(g)[0:2]``, ``step(g) = rint(d * 2^10)`` (half to even) as two int32, ``contact(g) = s``. A
   non-finite value among the eight heights or the four coordinates read, or ``|d * 2^10| >= 2^31`` (in fp64 also a value just
   under the bound that rounds to it; fp32 has none): ``step(g) = (0, 0)`` and ``contact(g) = -1``. Frame 0 of a video: ``step = (0, 0)``, ``contact = argmin_k h_k(0)``, -1 when a height is not finite.
   The choice has no hysteresis: flipping between two planted joints is harmless, both give the same step up to their own
   motion. Comparisons, never min / max: a NaN is seen.
3. Offset. ``S(g) = S(g - 1) + step(g)`` in int64, ``S(-1) = (0, 0)``; the quantum is ``2^-10`` of the length unit. The running
   sum is an integer sum: exact, associative, independent of grid, tiling and chunking. No floating-point value is ever summed
   across frames.
4. Output root row. ``x <- float(fp64(x) + S_x(g) * 2^-10)`` and y likewise; z unchanged, or with ``ground=z0`` (CARLA's z)
   ``z <- z + (z0 - min_k h_k(g))`` in the rows' dtype: the lowest contact then sits on the plane in EVERY frame -- there are no
   flight phases, a jump is pressed onto the ground (a frame with a non-finite height gets a NaN z). The three angles are
   copied bit for bit. The bones are not rewritten.
5. Carried state ``(S (N,2) int64, points (N,4,3))``: the offset after the last frame and that frame's four ``p_k``. A step is a
   pure function of two frames' rows and the sum an integer one, so a video pushed in chunks of any length gives the uncut
   video's bits. Each clip of a batch is a video of its own unless ``push`` is used.
"""
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON, PARENTS
from pedestrians_video_2_carla_amd.walker_control.resample import check_rows

CONTACTS = (CARLA_SKELETON.crl_foot__R.value, CARLA_SKELETON.crl_toe__R.value, CARLA_SKELETON.crl_foot__L.value,
            CARLA_SKELETON.crl_toe__L.value)
BONES = len(PARENTS)
QUANTUM = 2.0 ** -10
STEP_BOUND = 2.0 ** 31
WANT = ('root', 'steps', 'contact')
MAPPINGS = {None: 0, 'auto': 0, 'per_video': 1, 'frame_parallel': 2, 0: 0, 1: 1, 2: 2}


def _chain() -> Tuple[int, ...]:
    """The contact joints and their ancestors, parents first (``PARENTS`` is in depth-first order)."""
    need = set()
    for j in CONTACTS:
        while j >= 0:
            need.add(j)
            j = PARENTS[j]
    return tuple(sorted(need))


CHAIN = _chain()


def check_mapping(mapping) -> int:
    if isinstance(mapping, bool) or mapping not in MAPPINGS:
        raise ValueError(f"root_motion: mapping {mapping!r}; None, 'auto', 'per_video' (1) or 'frame_parallel' (2) expected")
    return MAPPINGS[mapping]


def check_want(want: Sequence[str]) -> Tuple[str, ...]:
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in WANT for w in want):
        raise ValueError(f'root_motion: want = {want}; some of {WANT} expected')
    return want


def check_ground(ground) -> Optional[float]:
    if ground is None:
        return None
    z0 = float(ground)
    if z0 != z0 or z0 in (float('inf'), float('-inf')) or not torch.isfinite(torch.tensor(z0, dtype=torch.float32)):
        raise ValueError(f'root_motion: ground = {ground}; a finite height expected')
    return z0


def check_state(bones: Tensor, state, first_frame: int, what: str = 'root_motion_carla_rows'):
    """The carried ``(S (N,2) int64, points (N,4,3) like the bones)`` or None; frames that continue a video need it."""
    if first_frame < 0:
        raise ValueError(f'{what}: first_frame = {first_frame} is negative')
    if state is None:
        if first_frame > 0:
            raise ValueError(f'{what}: frames from {first_frame} on continue a video: the state after frame {first_frame - 1} is needed')
        return None
    if not isinstance(state, (tuple, list)) or len(state) != 2:
        raise ValueError(f'{what}: state = (S (N,2) int64, points (N,4,3)) expected')
    S, pts = state
    N = bones.shape[0]
    if not isinstance(S, Tensor) or tuple(S.shape) != (N, 2) or S.dtype != torch.int64 or S.device != bones.device:
        raise ValueError(f'{what}: state offset {getattr(S, "shape", None)} {getattr(S, "dtype", None)}; ({N},2) int64 on the '
                         "bones' device expected")
    if not isinstance(pts, Tensor) or tuple(pts.shape) != (N, 4, 3) or pts.dtype != bones.dtype or pts.device != bones.device:
        raise ValueError(f'{what}: state points {getattr(pts, "shape", None)} {getattr(pts, "dtype", None)}; ({N},4,3) like the '
                         'bones expected')
    return S, pts


def check_bones(bones: Tensor, root: Optional[Tensor], what: str = 'root_motion_carla_rows'):
    check_rows(bones, root, None, what)
    if bones.shape[-2] != BONES:
        raise ValueError(f'{what}: {bones.shape[-2]} bones; the {BONES} of the CARLA skeleton expected (there is no other tree)')
    if not bones.dtype.is_floating_point:
        raise ValueError(f'{what}: bones of {bones.dtype}; a floating-point dtype expected')


# ---- the definition on tensor ops: every product and sum written out, so a frame's bits do not depend on the batch around it ----
def _pose(rows: Tensor):
    """(...,6) rows -> the location as 3 tensors and the matrix as 9 (row-major), the closed form of Rx(a0) Ry(a1) Rz(a2)."""
    x, y, z, pitch, yaw, roll = rows.unbind(-1)
    a0, a1, a2 = torch.deg2rad(-roll), torch.deg2rad(-pitch), torch.deg2rad(-yaw)
    s0, c0, s1, c1, s2, c2 = torch.sin(a0), torch.cos(a0), torch.sin(a1), torch.cos(a1), torch.sin(a2), torch.cos(a2)
    rot = (c1 * c2, -(c1 * s2), s1,
           c0 * s2 + (s0 * s1) * c2, c0 * c2 - (s0 * s1) * s2, -(s0 * c1),
           s0 * s2 - (c0 * s1) * c2, s0 * c2 + (c0 * s1) * s2, c0 * c1)
    return (x, y, -z), rot


def _vmul(v, a):
    """Row vector times matrix."""
    return tuple(v[0] * a[k] + (v[1] * a[3 + k] + v[2] * a[6 + k]) for k in range(3))


def _mul(a, b):
    return tuple(a[i * 3] * b[k] + (a[i * 3 + 1] * b[3 + k] + a[i * 3 + 2] * b[6 + k]) for i in range(3) for k in range(3))


def contact_points(bones: Tensor, root: Optional[Tensor]) -> Tensor:
    """``p_k`` (N,T,4,3) of step 1, in the dtype of ``bones``."""
    if root is None:
        root = torch.zeros(tuple(bones.shape[:2]) + (6,), dtype=bones.dtype, device=bones.device)
    loc, rot = _pose(bones)
    x, A = {}, {}
    for j in CHAIN:
        lj, Rj, p = tuple(c[..., j] for c in loc), tuple(m[..., j] for m in rot), PARENTS[j]
        if p < 0:
            x[j], A[j] = lj, Rj
        else:
            x[j] = tuple(u + v for u, v in zip(_vmul(lj, A[p]), x[p]))
            A[j] = _mul(Rj, A[p])
    r, W = _pose(root)
    return torch.stack([torch.stack([u + v for u, v in zip(_vmul(x[j], W), r)], -1) for j in CONTACTS], -2)


def _lowest(h: Tensor) -> Tuple[Tensor, Tensor]:
    """(...,4) -> the smallest value and the smallest index that has it, by comparisons in ascending k."""
    best, at = h[..., 0], torch.zeros(h.shape[:-1], dtype=torch.int64, device=h.device)
    for k in range(1, h.shape[-1]):
        less = h[..., k] < best
        best, at = torch.where(less, h[..., k], best), torch.where(less, torch.full_like(at, k), at)
    return best, at


def frame_steps(points: Tensor, before: Optional[Tensor]):
    """``points`` (N,T,4,3), ``before`` (N,4,3) the points of the frame before the first or None when that is frame 0 of the
    videos -> ``(steps (N,T,2) int32, contact (N,T) int8, lowest (N,T), margin (N,T))``: ``lowest`` is ``min_k h_k`` (NaN with a
    non-finite height), ``margin`` the gap between the best and the second-best ``m_k`` (infinite at a video's frame 0)."""
    N, T = points.shape[:2]
    h = -points[..., 2]
    fin = torch.isfinite(h).all(-1)
    low, at = _lowest(h)
    low = torch.where(fin, low, torch.full_like(low, float('nan')))
    first = points[:, :1] if before is None else before.unsqueeze(1)          # frame 0 of a video: a stand-in, overwritten below
    prev = torch.cat((first, points[:, :-1]), 1)
    hp = -prev[..., 2]
    m = torch.where(hp > h, hp, h)
    best, s = _lowest(m)
    pick = s[..., None, None].expand(N, T, 1, 3)
    ps, cs = prev.gather(2, pick)[..., 0, :2], points.gather(2, pick)[..., 0, :2]
    v = (ps - cs) * (1.0 / QUANTUM)
    ok = (fin & torch.isfinite(hp).all(-1) & torch.isfinite(ps).all(-1) & torch.isfinite(cs).all(-1)
          & (v.abs() < STEP_BOUND).all(-1) & (torch.round(v).abs() < STEP_BOUND).all(-1))  # the latter: fp64 just under the bound
    steps = torch.where(ok.unsqueeze(-1), torch.round(v), torch.zeros_like(v)).to(torch.int32)
    contact = torch.where(ok, s, torch.full_like(s, -1))
    rest = torch.where(torch.arange(4, device=m.device) == s.unsqueeze(-1), torch.full_like(m, float('inf')), m)
    margin = _lowest(rest)[0] - best
    if before is None and T > 0:
        steps[:, 0] = 0
        contact[:, 0] = torch.where(fin[:, 0], at[:, 0], torch.full_like(at[:, 0], -1))
        margin[:, 0] = float('inf')
    return steps, contact.to(torch.int8), low, margin


@torch.no_grad()
def root_motion_rows(bones: Tensor, root: Optional[Tensor], ground: Optional[float], state, first_frame: int) -> Dict[str, Tensor]:
    """The definition, on the tensors' device and in their dtype, behind the checks of ``ops.root_motion_carla_rows``: all of
    ``root``, ``steps``, ``contact`` and ``state``."""
    N, T = bones.shape[:2]
    rows = root if root is not None else torch.zeros((N, T, 6), dtype=bones.dtype, device=bones.device)
    if first_frame == 0:                                                      # nothing lies before the first frame of a video
        state = None
    offset = state[0] if state is not None else torch.zeros((N, 2), dtype=torch.int64, device=bones.device)
    if T == 0:
        return {'root': rows.clone(), 'steps': torch.zeros((N, 0, 2), dtype=torch.int32, device=bones.device),
                'contact': torch.zeros((N, 0), dtype=torch.int8, device=bones.device), 'state': state}
    points = contact_points(bones, rows)
    steps, contact, low, _ = frame_steps(points, state[1] if state is not None else None)
    S = offset.unsqueeze(1) + torch.cumsum(steps.to(torch.int64), 1)
    out = rows.clone()
    out[..., :2] = (rows[..., :2].double() + S.double() * QUANTUM).to(rows.dtype)
    if ground is not None:
        out[..., 2] = rows[..., 2] + (torch.tensor(ground, dtype=rows.dtype, device=rows.device) - low)
    return {'root': out, 'steps': steps, 'contact': contact, 'state': (S[:, -1].clone(), points[:, -1].clone())}


# ---- the streaming class -------------------------------------------------------------------------------------------------------
class CarlaRootMotion:
    """``CarlaRootMotion(ground=None).apply(bones, root)`` -> ``(bones, root)`` with the root rows of planted feet: every clip a
    video of its own, stateless. ``push(bones, root)`` / ``reset()`` stream the same N videos chunk by chunk (any chunk length
    >= 1): every push returns its chunk's frames, and the concatenated outputs are those of the uncut video, bit for bit. The
    state is ``(S (N,2) int64, points (N,4,3))`` on the videos' device and the count of frames seen. The bones come back as they
    were given. ``ground``: CARLA's z of a plane the lowest contact joint is put on in every frame (no flight phases)."""

    def __init__(self, ground=None):
        self.ground = check_ground(ground)
        self.reset()

    def reset(self):
        """The next ``push`` starts new videos."""
        self._state = None
        self._layout = None
        self.frames = 0          # frames seen: the global index of the next chunk's first frame

    def apply(self, bones: Tensor, root: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        return bones, ops.root_motion_carla_rows(bones, root, ground=self.ground)['root']

    def push(self, bones: Tensor, root: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        check_bones(bones, root, 'CarlaRootMotion.push')
        N, T = bones.shape[:2]
        if T < 1:
            raise ValueError('CarlaRootMotion.push: a chunk holds at least one frame')
        layout = (N, root is not None, bones.dtype, bones.device)
        if self._layout is not None and layout != self._layout:
            raise RuntimeError(f'CarlaRootMotion.push: (videos, root, dtype, device) = {layout} after {self._layout}; '
                               'reset() starts other videos')
        out = ops.root_motion_carla_rows(bones, root, ground=self.ground, state=self._state, first_frame=self.frames)
        self._state = out['state']
        self._layout = layout
        self.frames += T
        return bones, out['root']


def as_root_motion(root_motion) -> Optional[CarlaRootMotion]:
    """None or False, True (the defaults), a dict of ``CarlaRootMotion``'s arguments, or an instance -> the instance or None."""
    if root_motion is None or root_motion is False:
        return None
    if root_motion is True:
        return CarlaRootMotion()
    if isinstance(root_motion, CarlaRootMotion):
        return root_motion
    if isinstance(root_motion, dict):
        try:
            return CarlaRootMotion(**root_motion)
        except TypeError as e:
            raise ValueError(f'root_motion: {e}') from None
    raise ValueError('root_motion: None, True, a CarlaRootMotion or a dict of its arguments expected')
