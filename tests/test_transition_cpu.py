"""Keyframed level-set colliders, the parts that need no GPU: the ctypes mirror of zs_rocm_levelset_transition against the header, the
queue semantics of LevelSetSequence, and the float64 restatement (tests/ref64_transition.py) on its own: that it tells two phases apart
and that the GPU tests' case satisfies the conditions their bounds rest on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref64_transition as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_mirror_of_the_transition_struct_matches_the_header(tmp_path):
    """every field of _lib.LevelSetTransition at the offset and of the size the host compiler gives the member of the same name, same
    total size (the method of test_levelset_cpu.py); the level-set struct inside it is the one the single level-set entries take"""
    from zpc_amd import _lib
    pairs = {"zs_rocm_levelset_transition": _lib.LevelSetTransition, "zs_rocm_levelset": _lib.LevelSet}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "zs_rocm.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append('  printf("%s|size|%%zu|0\\n", sizeof(%s));' % (cname, cname))
        for m, _ in cls._fields_:
            src.append('  printf("%s|%s|%%zu|%%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, m, cname, m, cname, m))
    src += ['  return 0;', '}']
    c = tmp_path / "mirror.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "mirror"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        sname, m, a, b = line.split("|")
        got.setdefault(sname, {})[m] = [int(a), int(b)]
    for cname, cls in pairs.items():
        assert C.sizeof(cls) == got[cname]["size"][0], (cname, C.sizeof(cls), got[cname]["size"][0])
        for m, _ in cls._fields_:
            f = getattr(cls, m)
            assert [f.offset, f.size] == got[cname][m], (cname, m, [f.offset, f.size], got[cname][m])
    assert [m for m, _ in _lib.LevelSetTransition._fields_] == ["src", "dst", "stepDt", "alpha", "maxSpeed"]


class _Frame:
    """what LevelSetSequence asks of a keyframe, without a device"""

    def __init__(self, name, speed=0.0, band=0.1, background=0.1, has_velocity=True):
        from zpc_amd._lib import LevelSet
        self.name, self.speed, self.band, self.background, self.has_velocity = name, speed, band, background, has_velocity
        self.view = LevelSet()
        self.view.h = 1.0
        self.view.numChannels = int(name)      # (a tag to recognise the struct by)

    def max_speed(self):
        return self.speed


def test_sequence_queue_semantics():
    from zpc_amd.levelset import LevelSetSequence, POP_THRESHOLD
    f32 = np.float32
    assert POP_THRESHOLD == f32(1) - f32(128) * f32(2.0 ** -23)
    seq = LevelSetSequence(None, 0.01)
    with pytest.raises(RuntimeError):
        seq.view()                                   # an empty queue raises
    a, b, c = _Frame(1, speed=2.0), _Frame(2, speed=3.0, background=5.0), _Frame(3)
    seq.push(a)
    v = seq.view()
    assert len(seq) == 1 and v.src.numChannels == 1 and v.dst.numChannels == 1      # one keyframe: dst = src
    assert v.alpha == 0.0 and v.stepDt == f32(0.01) and v.maxSpeed == f32(2.0)
    seq.push(b)
    seq.push(c)
    v = seq.view()
    assert (v.src.numChannels, v.dst.numChannels) == (1, 2) and v.maxSpeed == 5.0    # cells and |background| of both keyframes
    # the pop threshold, in float32: alpha = 1 - 128 eps stays, the next float above it wraps and pops
    seq.advance(POP_THRESHOLD)
    assert seq.alpha == POP_THRESHOLD and len(seq) == 3
    seq.alpha = f32(0)
    seq.advance(np.nextafter(POP_THRESHOLD, f32(2)))
    assert len(seq) == 2 and seq.alpha == f32(np.nextafter(POP_THRESHOLD, f32(2)) - f32(1)) and seq.alpha < 0
    seq.alpha = f32(0)
    for _ in range(4):
        seq.advance(0.25)                            # 0.25 four times is exactly 1 > threshold: one pop, alpha 0
    assert len(seq) == 1 and seq.alpha == 0 and seq.view().src.numChannels == 3
    seq.advance(2.5)                                 # pops twice; an empty queue is left alone by the second
    assert len(seq) == 0 and seq.alpha == f32(0.5)
    seq.set_step_dt(0.5)
    assert seq.step_dt == 0.5
    with pytest.raises(ValueError):
        seq.set_step_dt(-1.0)


def test_sequence_push_checks_the_band():
    from zpc_amd.levelset import LevelSetSequence
    seq = LevelSetSequence(None, 0.01)
    seq.push(_Frame(1, speed=9.9, band=0.1))         # 0.099 <= 0.1
    with pytest.raises(ValueError):
        seq.push(_Frame(2, speed=10.5, band=0.1))    # 0.105 > 0.1
    with pytest.raises(ValueError):
        seq.push(_Frame(2, speed=1.0, band=0.1, background=11.0))   # the background is a "v" value too
    assert len(seq) == 1
    seq.push(_Frame(2, speed=10.5, band=0.1), allow_wide=True)
    seq.push(_Frame(3, speed=1e9, band=0.1, has_velocity=False))    # no "v": speed 0
    seq.push(_Frame(4, speed=1e9, band=None))                        # band unknown: not checked
    assert len(seq) == 4


def test_reference_separates_two_phases():
    """negative control: at the same points the restatement's distance at alpha = 0 and at alpha = 0.5 differ by more than the sum of the
    two bounds on at least half of the inside points -- a kernel that ignored alpha (or the advection) would fail the GPU comparison"""
    frames = rt.keyframes()
    x = rt.material_points(0.25).astype(np.float32)
    s0, b0 = rt.reference(frames, 0.0).sdf(x)
    s5, b5 = rt.reference(frames, 0.5).sdf(x)
    inside = s0 < 0
    apart = np.abs(s0 - s5) > b0 + b5
    # without the advection (stepDt = 0) the blend at 0.5 is another function again
    n5, bn5 = rt.reference(frames, 0.5, step_dt=0.0).sdf(x)
    apart_adv = np.abs(n5 - s5) > bn5 + b5
    print("TRANSITION control: %d inside, %.3f of them apart in alpha, %.3f apart in the advection" %
          (inside.sum(), apart[inside].mean(), apart_adv[inside].mean()))
    assert inside.sum() > 1000
    assert apart[inside].mean() >= 0.5 and apart_adv[inside].mean() >= 0.5


@pytest.mark.parametrize("vel", ["both", "dst_only"])
@pytest.mark.parametrize("alpha", rt.ALPHAS)
def test_input_conditions_of_the_gpu_case(alpha, vel):
    """on the reference alone, fixed seed: no stencil of any sample of either level set touches an absent block (so the uniform "v" is
    never blended with the background), and at most 1 % of the inside points have a per-keyframe gradient length below 0.5 (those are
    left out of the normal and slip checks)"""
    frames = rt.keyframes(vel_src=vel == "both")
    ref = rt.reference(frames, alpha)
    x = rt.material_points(alpha).astype(np.float32)
    keys = {id(ref.src): frames[0][0], id(ref.dst): frames[1][0]}
    for ls, p in ref.sample_positions(x):
        assert not rt.touches_absent(ls, keys[id(ls)], p).any()
    sd, b = ref.sdf(x)
    inside = sd < 0
    _, _, l = ref.normal(x[inside])
    assert inside.sum() > 1000 and (~inside).sum() > 1000
    assert (np.abs(sd) <= 2.5 * rt.VOXEL).all()
    assert (l < 0.5).mean() <= 0.01
