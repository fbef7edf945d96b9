"""pose_changes (reference loss/pose_changes.py:7-28) on the host -- its registry entry, the flow resolving it, the tensor path
against the written-out sum of squares on the golden pose changes of losses_extra.npz, the cases it declines -- and the C ABI of
K27 (csrc/p2c_pose_change_loss.hip): symbols declared, bound and exported, the descriptor's layout against the header."""
import ctypes
import os
import re
import subprocess

import torch

from pedestrians_video_2_carla_amd.loss import LossModes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K27_SYMBOLS = ('p2c_pose_change_loss_workspace_floats', 'p2c_pose_change_loss_fwd', 'p2c_pose_change_loss_bwd')


def test_pose_changes_is_registered_with_a_summing_mse():
    fn, crit = LossModes.pose_changes.value
    assert callable(fn) and type(crit) is torch.nn.MSELoss and crit.reduction == 'sum'
    names = list(LossModes.__members__)
    assert names.index('pose_changes') == names.index('cum_pose_changes') + 1        # the reference's position


def test_flow_resolves_pose_changes():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON), loss_modes=['pose_changes'])
    assert [n for (n, *_r) in flow._losses_to_calculate] == ['pose_changes']
    assert flow._pose_change_only()
    both = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                              loss_modes=['loc_2d_3d', 'cum_pose_changes'])
    assert [n for (n, *_r) in both._losses_to_calculate] == ['loc_2d', 'loc_3d', 'loc_2d_3d', 'cum_pose_changes']
    assert not both._pose_change_only() and both._fusable(None)       # the location losses keep their lean launches


def test_pose_changes_is_the_sum_of_squares_on_the_host(golden):
    from oracle.pose_head import rotation_6d_to_matrix
    g = golden('losses_extra')
    fn, crit = LossModes.pose_changes.value
    for dtype, rtol in ((torch.float32, 1e-5), (torch.float64, 1e-12)):
        pred, tgt = g['cum_pred'].to(dtype), g['cum_tgt'].to(dtype)
        p = pred.clone().requires_grad_(True)
        loss = fn(criterion=crit, pose_inputs=p, targets={'pose_changes': tgt})
        assert loss.dtype == dtype
        torch.testing.assert_close(loss.double(), ((pred.double() - tgt.double()) ** 2).sum(), rtol=rtol, atol=0)
        loss.backward()
        torch.testing.assert_close(p.grad.double(), 2 * (pred.double() - tgt.double()), rtol=rtol, atol=1e-12)
        # the raw 6-D network output = the first two rows: compared as the matrices the reference's mixin makes of it
        six = pred[..., :2, :].reshape(*pred.shape[:3], 6)
        got = fn(criterion=crit, pose_inputs=six, targets={'pose_changes': tgt})
        want = ((rotation_6d_to_matrix(six.double()) - tgt.double()) ** 2).sum()
        torch.testing.assert_close(got.double(), want, rtol=rtol, atol=0)
        # the golden predictions are rotations to fp32 rounding, so this is the matrix form's value too (the rtol
        # tests/test_losses_extra.py applies to the 6-D form of cum_pose_changes)
        torch.testing.assert_close(got.double(), ((pred.double() - tgt.double()) ** 2).sum(), rtol=1e-4, atol=0)
    # another criterion is applied as it is
    l1 = fn(criterion=torch.nn.L1Loss(), pose_inputs=g['cum_pred'], targets={'pose_changes': g['cum_tgt']})
    torch.testing.assert_close(l1, (g['cum_pred'] - g['cum_tgt']).abs().mean())


def test_pose_changes_declines_what_it_cannot_compare(golden):
    g = golden('losses_extra')
    fn, crit = LossModes.pose_changes.value
    pred, tgt = g['cum_pred'], g['cum_tgt']
    assert fn(criterion=crit, targets={'pose_changes': tgt}) is None                               # no pose_inputs
    assert fn(criterion=crit, pose_inputs=None, targets={'pose_changes': tgt}) is None
    assert fn(criterion=crit, pose_inputs=(pred, pred), targets={'pose_changes': tgt}) is None      # (changes, absolute rotations)
    assert fn(criterion=crit, pose_inputs=pred[..., 0], targets={'pose_changes': tgt}) is None      # a location output (B,T,J,3)
    assert fn(criterion=crit, pose_inputs=pred, targets={}) is None
    assert fn(criterion=crit, pose_inputs=pred, targets=None) is None
    # keyword arguments of the other losses are accepted and ignored
    assert fn(criterion=crit, pose_inputs=pred, targets={'pose_changes': tgt}, projection_2d=None, requirements={}) is not None


def test_host_tensors_and_other_criteria_stay_on_the_tensor_path(golden, monkeypatch):
    from pedestrians_video_2_carla_amd import ops
    g = golden('losses_extra')
    pred, tgt = g['cum_pred'], g['cum_tgt']
    assert not ops.pose_change_loss_supported(pred, tgt, torch.nn.MSELoss())                        # host tensors
    calls = []
    monkeypatch.setattr(ops, 'pose_change_loss', lambda *a, **k: calls.append(a))
    for mode in ('pose_changes', 'cum_pose_changes'):
        fn, crit = LossModes[mode].value
        assert fn(criterion=crit, pose_inputs=pred, targets={'pose_changes': tgt}) is not None
    assert not calls


def _lib_loaded():
    from pedestrians_video_2_carla_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_k27_symbols_are_declared_bound_and_exported():
    _lib, lib = _lib_loaded()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    for name in K27_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
    for name in K27_SYMBOLS[1:]:                             # the stream goes last: the LDS-poisoning audit wrapper covers them
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p
    assert _lib.SYMBOLS[K27_SYMBOLS[0]][0] is ctypes.c_int64


def test_k27_descriptor_layout_matches_the_header(tmp_path):
    from pedestrians_video_2_carla_amd._lib import PoseChangeLossDesc
    fields = [f[0] for f in PoseChangeLossDesc._fields_]
    src = tmp_path / 'pcl.c'
    body = '\n'.join(f'  printf("{f} %zu\\n", offsetof(p2c_pose_change_loss_desc, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(p2c_pose_change_loss_desc));\n' + body + '\n  return 0;\n}\n')
    exe = tmp_path / 'pcl'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(PoseChangeLossDesc)
    for f in fields:
        assert int(out[f]) == getattr(PoseChangeLossDesc, f).offset, f


def test_k27_refuses_bad_arguments_without_a_device():
    """Every refusal is answered on the host, before anything could be launched: these run on a machine without a GPU."""
    _lib, lib = _lib_loaded()

    def desc(B=2, T=3, J=4, six=0, cum=1, mean=1, max_blocks=0, **ptrs):
        d = _lib.PoseChangeLossDesc()
        d.B, d.T, d.J, d.pred_is_6d, d.cumulative, d.mean, d.max_blocks = B, T, J, six, cum, mean, max_blocks
        for f in ('pred', 'target', 'workspace', 'loss', 'grad_loss', 'grad_pred'):
            setattr(d, f, ptrs.get(f, 64))
        return ctypes.byref(d)
    for fn in (lib.p2c_pose_change_loss_fwd, lib.p2c_pose_change_loss_bwd):
        assert fn(None, None) == -1
        for f in ('pred', 'target', 'workspace'):
            assert fn(desc(**{f: None}), None) == -1, f
        assert fn(desc(T=0), None) == -2 and fn(desc(J=0), None) == -2 and fn(desc(B=-1), None) == -2
        assert fn(desc(max_blocks=-1), None) == -2
        for flag in ('six', 'cum', 'mean'):
            assert fn(desc(**{flag: 2}), None) == -3 and fn(desc(**{flag: -1}), None) == -3, flag
        # 32-bit element indices: B T J 9 >= 2^31 is refused, the last size below it is not (B = 0 there: nothing to launch)
        assert fn(desc(B=238609295, T=1, J=1), None) == -2 and fn(desc(B=1 << 40, T=1 << 20, J=1 << 20), None) == -2
        assert fn(desc(B=9177281, T=1, J=26), None) == -2 and fn(desc(B=1, T=1 << 16, J=1 << 16), None) == -2
        assert fn(desc(B=0), None) == 0
    assert lib.p2c_pose_change_loss_fwd(desc(loss=None), None) == -1
    assert lib.p2c_pose_change_loss_bwd(desc(grad_pred=None), None) == -1
    assert lib.p2c_pose_change_loss_bwd(desc(grad_loss=None), None) == -1
    assert lib.p2c_pose_change_loss_fwd(desc(six=1, pred=68), None) == -2                # 6-D rows move as 8-byte words
    ws = lib.p2c_pose_change_loss_workspace_floats
    assert ws(None) == -1 and ws(desc(T=0)) == -2 and ws(desc(cum=3)) == -3 and ws(desc(B=238609295, T=1, J=1)) == -2
    sizes = [ws(desc(B=B, T=16, J=26)) for B in (0, 1, 2, 256, 8192)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert sizes[3] >= 2 * 9 * 256 * 16 * 26                 # the differences and the running products of every frame
    assert ws(desc(B=238609294, T=1, J=1)) >= 2 * 9 * 238609294
