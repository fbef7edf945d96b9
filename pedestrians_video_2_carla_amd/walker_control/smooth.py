"""CARLA rows smoothed along time: the definition of K39 and the streaming smoother on top of ``ops.smooth_carla_rows``.

Every converter (K30, K32, K35, K36) makes a frame's rows from that frame alone, from models trained on noisy keypoints: a played
animation jitters. The rows -- ``bones`` (N,T,J,6) and ``root`` (N,T,6), each (x, y, z, pitch, yaw, roll) -- cannot be averaged as
they are: Euler angles are wrong across the +-180 degree seam and near +-90 degrees of pitch. Rotations are therefore filtered as
the unit quaternions ``resample._row_quat`` makes of the rows (K37's) and read back through ``resample._quat_rows``.
Comparisons, never min / max: a NaN goes where the arithmetic takes it and nowhere else.

``mode='gaussian'``, offline and zero-phase. ``sigma`` in frames, radius ``R`` (default ``ceil(3 sigma)``, 0 <= R <= 32), weights
``w[d] = float32(exp(-d^2 / (2 sigma^2)))`` formed once in fp64 on the host (``gauss_table``): the definition and the kernel read
the same table. Output frame t, a global index counted from the start of the video, combines source frames
``max(0, t - R) .. min(t + R, g_last)``: the window is truncated at the real ends of the video and only there. Locations are
``sum(w x) / sum(w)``; every neighbour's quaternion is negated when its dot product with the centre frame's is < 0, and the
rotation is the normalised ``sum(w q)``; all sums in ascending frame order. ``R == 0`` or ``sigma == 0``: the rows, copied.

``mode='one_euro'``, causal (Casiez, Roussel, Vogel: the 1-euro filter, CHI 2012). ``alpha(fc) = 1 / (1 + fps / (2 pi fc))``.
Frame 0 of a video sets ``x^ = x``, ``v^ = 0``, ``q^`` = the row's quaternion, ``w^ = 0`` and its row is copied. Frame t:
``v = (x - x^) fps``, ``v^ += alpha(d_cutoff) (v - v^)``, ``x^ += alpha(min_cutoff + beta_loc |v^|) (x - x^)``; ``q`` on ``q^``'s
hemisphere, ``d = q^ . q`` clamped to <= 1, ``w = 2 acos(d) fps``, ``w^ += alpha(d_cutoff) (w - w^)``,
``q^ = slerp(q^, q, alpha(min_cutoff + beta_rot w^))`` with K37's weights (lerp above d = 0.99999), normalised. The state of a row
is ``(x^ 3, v^ 3, q^ 4, w^ 1)`` padded to 12 values; it is carried as it is and never re-read from an output row, which is what
makes a cut video give the uncut video's bits. ``fps / (2 pi)`` and ``alpha(d_cutoff)`` are formed in fp64 and used in the rows'
dtype.
"""
import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.walker_control.resample import LERP_ABOVE, _quat_rows, _row_quat, check_rows

MODES = ('gaussian', 'one_euro')
MAX_RADIUS = 32
STATE = 12
TWO_PI = 2.0 * math.pi


def check_mode(mode: str) -> str:
    if mode not in MODES:
        raise ValueError(f'smooth: mode {mode!r}; one of {MODES} expected')
    return mode


def gauss_params(sigma, radius=None) -> Tuple[float, int]:
    """``(sigma, R)`` checked; ``R`` defaults to ``ceil(3 sigma)``, and ``sigma == 0`` is ``R = 0``: the identity."""
    if sigma is None:
        raise ValueError("smooth: mode 'gaussian' needs sigma (in frames)")
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f'smooth: sigma = {sigma}; a finite value >= 0 expected')
    R = int(math.ceil(3.0 * sigma)) if radius is None else int(radius)
    if radius is not None and R != radius:
        raise ValueError(f'smooth: radius = {radius}; a whole number expected')
    if not 0 <= R <= MAX_RADIUS:
        raise ValueError(f'smooth: radius = {R} lies outside 0..{MAX_RADIUS}'
                         + (' (the default ceil(3 sigma): give a radius)' if radius is None else ''))
    return sigma, (0 if sigma == 0.0 else R)


def gauss_table(sigma: float, R: int) -> Tensor:
    """``float32(exp(-d^2 / (2 sigma^2)))`` for d = 0..R, formed in fp64, on the host."""
    if R == 0:
        return torch.ones(1, dtype=torch.float32)
    return torch.tensor([math.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(R + 1)], dtype=torch.float64).to(torch.float32)


def euro_params(fps, min_cutoff=1.0, beta_loc=0.0, beta_rot=0.0, d_cutoff=1.0) -> Dict[str, float]:
    if fps is None:
        raise ValueError("smooth: mode 'one_euro' needs fps")
    p = dict(fps=float(fps), min_cutoff=float(min_cutoff), beta_loc=float(beta_loc), beta_rot=float(beta_rot),
             d_cutoff=float(d_cutoff))
    for k in ('fps', 'min_cutoff', 'd_cutoff'):
        v32 = float(torch.tensor(p[k], dtype=torch.float32))
        if not (math.isfinite(p[k]) and p[k] > 0.0 and math.isfinite(v32) and v32 > 0.0):
            raise ValueError(f'smooth: {k} = {p[k]}; a positive finite value expected')
    for k in ('beta_loc', 'beta_rot'):
        if not (math.isfinite(p[k]) and p[k] >= 0.0 and math.isfinite(float(torch.tensor(p[k], dtype=torch.float32)))):
            raise ValueError(f'smooth: {k} = {p[k]}; a finite value >= 0 expected')
    return p


def check_state(bones: Tensor, root: Optional[Tensor], state, what: str = 'smooth_carla_rows'):
    """The carried one-euro state ``(bones (N,J,12), root (N,12) or None)`` or None; returns ``(state_bones, state_root)``."""
    if state is None:
        return None, None
    sb, sr = state if isinstance(state, (tuple, list)) else (state, None)
    N, _, J, _ = bones.shape
    if sb is None or tuple(sb.shape) != (N, J, STATE) or sb.dtype != bones.dtype or sb.device != bones.device:
        raise ValueError(f'{what}: state of the bones {None if sb is None else tuple(sb.shape)}; ({N},{J},{STATE}) like the bones expected')
    if root is not None and (sr is None or tuple(sr.shape) != (N, STATE) or sr.dtype != bones.dtype or sr.device != bones.device):
        raise ValueError(f'{what}: state of the root {None if sr is None else tuple(sr.shape)}; ({N},{STATE}) like the root expected')
    return sb, (sr if root is not None else None)


def gauss_span(first_output: int, count: int, R: int, last_frame: int) -> Tuple[int, int]:
    """The smallest and the largest global source frame the outputs' windows read (``last_frame < 0``: not known yet)."""
    hi = first_output + count - 1 + R
    return max(first_output - R, 0), (hi if last_frame < 0 else min(hi, last_frame))


def check_gauss_span(first_output: int, count: int, R: int, first_frame: int, S: int, last_frame: int, what: str):
    if first_output < 0 or first_frame < 0 or count < 0 or last_frame < -1:
        raise ValueError(f'{what}: first_output, first_frame and count are not negative, last_frame is -1 or an index')
    if count == 0:
        return
    if last_frame >= 0 and first_output + count - 1 > last_frame:
        raise ValueError(f'{what}: outputs {first_output}..{first_output + count - 1} of a video that ends with frame {last_frame}')
    lo, hi = gauss_span(first_output, count, R, last_frame)
    if lo < first_frame or hi > first_frame + S - 1:
        raise ValueError(f'{what}: outputs {first_output}..{first_output + count - 1} read source frames {lo}..{hi}, '
                         f'frames {first_frame}..{first_frame + S - 1} are given')


# ---- the definition on tensor ops ----------------------------------------------------------------------------------------------
def _dot(a: Tensor, b: Tensor) -> Tensor:
    """(...,k) . (...,k) -> (...,1), the products added from the first to the last."""
    p = (a * b).unbind(-1)
    s = p[0]
    for v in p[1:]:
        s = s + v
    return s.unsqueeze(-1)


def _gauss_one(src: Tensor, table: Tensor, R: int, first_frame: int, first_output: int, count: int, last_frame: int) -> Tensor:
    """``src`` (N,S,...,6), global frames ``first_frame ..`` -> outputs ``first_output .. first_output + count - 1`` (N,count,...,6)."""
    S = src.shape[1]
    if R == 0 or count == 0:
        return src[:, first_output - first_frame:first_output - first_frame + count].clone()
    hi = first_frame + S - 1 if last_frame < 0 else min(last_frame, first_frame + S - 1)
    w = table.to(device=src.device, dtype=src.dtype)
    t = torch.arange(first_output, first_output + count, device=src.device)
    per_frame = (1, count) + (1,) * (src.ndim - 2)
    quat = _row_quat(src)
    centre = quat.index_select(1, (t - first_frame).clamp(0, S - 1))
    acc_l = torch.zeros(src.shape[:1] + (count,) + src.shape[2:-1] + (3,), dtype=src.dtype, device=src.device)
    acc_q = torch.zeros(acc_l.shape[:-1] + (4,), dtype=src.dtype, device=src.device)
    acc_w = torch.zeros(per_frame, dtype=src.dtype, device=src.device)
    for d in range(-R, R + 1):                                           # ascending frame order
        g = t + d
        used = ((g >= first_frame) & (g <= hi)).reshape(per_frame)      # frame 0 is not before first_frame: the span was checked
        idx = (g - first_frame).clamp(0, S - 1)
        loc, q = src.index_select(1, idx)[..., :3], quat.index_select(1, idx)
        q = torch.where(_dot(q, centre) < 0, -q, q)                      # on the centre's hemisphere
        acc_l = torch.where(used, acc_l + w[abs(d)] * loc, acc_l)
        acc_q = torch.where(used, acc_q + w[abs(d)] * q, acc_q)
        acc_w = torch.where(used, acc_w + w[abs(d)], acc_w)
    return _quat_rows(acc_l / acc_w, acc_q / torch.sqrt(_dot(acc_q, acc_q)))


@torch.no_grad()
def gauss_rows(bones: Tensor, root: Optional[Tensor], table: Tensor, R: int, first_frame: int, first_output: int, count: int,
               last_frame: int) -> Tuple[Tensor, Optional[Tensor]]:
    """The gaussian definition, on the tensors' device and in their dtype, behind the checks of ``ops.smooth_carla_rows``."""
    args = (table, R, first_frame, first_output, count, last_frame)
    return _gauss_one(bones, *args), (_gauss_one(root, *args) if root is not None else None)


def _euro_one(src: Tensor, state: Optional[Tensor], p: Dict[str, float]) -> Tuple[Tensor, Tensor]:
    """``src`` (N,T,...,6), ``state`` (N,...,12) or None -> the filtered rows and the state after the last frame."""
    fps, mc, k = p['fps'], p['min_cutoff'], p['fps'] / TWO_PI
    alpha_d = 1.0 / (1.0 + p['fps'] / (TWO_PI * p['d_cutoff']))
    if state is not None:
        hx, v, hq, om = state[..., 0:3], state[..., 3:6], state[..., 6:10], state[..., 10:11]
    outs = []
    for t in range(src.shape[1]):
        row = src[:, t]
        x, q = row[..., :3], _row_quat(row)
        if t == 0 and state is None:
            hx, v, hq, om = x, torch.zeros_like(x), q, torch.zeros_like(x[..., :1])
            outs.append(row)
            continue
        dx = x - hx
        v = v + alpha_d * (dx * fps - v)
        hx = hx + (1.0 / (1.0 + k / (mc + p['beta_loc'] * torch.sqrt(_dot(v, v))))) * dx
        d = _dot(hq, q)
        flip = d < 0
        q, d = torch.where(flip, -q, q), torch.where(flip, -d, d)
        d = torch.where(d > 1, torch.ones_like(d), d)
        theta = torch.acos(d)
        om = om + alpha_d * (2.0 * theta * fps - om)
        a = 1.0 / (1.0 + k / (mc + p['beta_rot'] * om))
        inv = 1.0 / torch.sin(theta)
        lerp = d > LERP_ABOVE
        wa = torch.where(lerp, 1.0 - a, torch.sin((1.0 - a) * theta) * inv)
        wb = torch.where(lerp, a, torch.sin(a * theta) * inv)
        s = wa * hq + wb * q
        hq = s / torch.sqrt(_dot(s, s))
        outs.append(_quat_rows(hx, hq))
    return torch.stack(outs, 1), torch.cat((hx, v, hq, om, torch.zeros_like(om)), -1)


@torch.no_grad()
def euro_rows(bones: Tensor, root: Optional[Tensor], state_bones: Optional[Tensor], state_root: Optional[Tensor],
              params: Dict[str, float]):
    """The one-euro definition: ``(bones, root or None, (state_bones, state_root or None))``; at least one frame."""
    out_b, new_b = _euro_one(bones, state_bones, params)
    if root is None:
        return out_b, None, (new_b, None)
    out_r, new_r = _euro_one(root, state_root, params)
    return out_b, out_r, (new_b, new_r)


# ---- the streaming smoother ----------------------------------------------------------------------------------------------------
class CarlaSmoother:
    """``CarlaSmoother(mode, **params).smooth(bones, root)``: every clip its own video, stateless. ``push(bones, root)`` /
    ``flush()`` / ``reset()`` stream the same N videos chunk by chunk (any chunk length >= 1), and the concatenated outputs are
    those of the uncut video, bit for bit. ``one_euro`` returns a chunk's T frames from every push and carries the state tensors;
    ``flush`` returns no frames. ``gaussian`` returns the frames whose windows are complete -- global index <= frames seen - 1 - R,
    possibly none and then without a launch -- and carries the last 2R source frames on their device; ``flush`` returns the rest,
    their windows truncated at the end that is now known. ``flush`` resets. ``params``: ``sigma``, ``radius`` /
    ``fps``, ``min_cutoff``, ``beta_loc``, ``beta_rot``, ``d_cutoff``."""

    def __init__(self, mode: str, **params):
        self.mode = check_mode(mode)
        try:
            if mode == 'gaussian':
                self.sigma, self.radius = gauss_params(**params)
                self.params = dict(sigma=self.sigma, radius=self.radius)
            else:
                self.params = euro_params(**params)
        except TypeError as e:
            raise ValueError(f'smooth: mode {mode!r}: {e}') from None
        self.reset()

    def reset(self):
        """The next ``push`` starts new videos."""
        self._carry = None       # gaussian: (bones (N,<=2R,J,6), root or None), the last source frames
        self._state = None       # one_euro: (state_bones, state_root or None)
        self._layout = None
        self._like = None        # an empty (N,0,J,6) / (N,0,6) pair of the videos' dtype and device
        self.frames = 0          # source frames seen: the global index of the next chunk's first frame
        self.outputs = 0         # outputs emitted: the global index of the next output

    def smooth(self, bones: Tensor, root: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        return ops.smooth_carla_rows(bones, root, mode=self.mode, **self.params)[:2]

    def push(self, bones: Tensor, root: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        check_rows(bones, root, None, 'CarlaSmoother.push')
        N, T, J, _ = bones.shape
        if T < 1:
            raise ValueError('CarlaSmoother.push: a chunk holds at least one frame')
        layout = (N, J, root is not None)
        if self._layout is not None and layout != self._layout:
            raise RuntimeError(f'CarlaSmoother.push: (videos, bones, root) = {layout} after {self._layout}; reset() starts other videos')
        if self.mode == 'one_euro':
            out_b, out_r, self._state = ops.smooth_carla_rows(bones, root, mode=self.mode, state=self._state, **self.params)
            total = self.frames + T
        else:
            R = self.radius
            if self._carry is not None:
                bones = torch.cat((self._carry[0], bones), 1)
                root = torch.cat((self._carry[1], root), 1) if root is not None else None
            seen = self.frames + T
            total = max(seen - R, 0) if R else seen
            out_b, out_r, _ = ops.smooth_carla_rows(bones, root, mode=self.mode, first_frame=seen - bones.shape[1],
                                                    first_output=self.outputs, count=total - self.outputs, last_frame=-1,
                                                    **self.params)
            keep = min(2 * R, bones.shape[1])
            self._carry = (bones[:, bones.shape[1] - keep:].detach().clone(),
                           root[:, root.shape[1] - keep:].detach().clone() if root is not None else None)
        self._like = (out_b[:, :0], out_r[:, :0] if out_r is not None else None)
        self._layout = layout
        self.frames += T
        self.outputs = total
        return out_b, out_r

    def flush(self) -> Tuple[Tensor, Optional[Tensor]]:
        """The frames still owed, now that the videos have ended; the smoother is reset."""
        if self._layout is None:
            raise RuntimeError('CarlaSmoother.flush: nothing was pushed')
        out = self._like
        if self.mode == 'gaussian' and self.outputs < self.frames:
            bones, root = self._carry
            out = ops.smooth_carla_rows(bones, root, mode=self.mode, first_frame=self.frames - bones.shape[1],
                                        first_output=self.outputs, count=self.frames - self.outputs, last_frame=self.frames - 1,
                                        **self.params)[:2]
        self.reset()
        return out


def as_smoother(smooth, fps=None) -> Optional[CarlaSmoother]:
    """None, a ``CarlaSmoother``, or a dict of its arguments (``mode`` among them; ``one_euro`` takes ``fps`` from the caller's
    when the dict has none) -> the smoother or None."""
    if smooth is None or isinstance(smooth, CarlaSmoother):
        return smooth
    if not isinstance(smooth, dict) or 'mode' not in smooth:
        raise ValueError("smooth: a CarlaSmoother or a dict of its arguments with 'mode' expected")
    args = dict(smooth)
    if args['mode'] == 'one_euro' and args.get('fps') is None and fps is not None:
        args['fps'] = fps
    return CarlaSmoother(**args)
