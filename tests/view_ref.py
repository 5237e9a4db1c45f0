"""ProgressiveViewHIP's display chain, restated once for every view rt_render can run:
mesh and sphere views, every display flag.  `run_view` makes one `rt_render --events` run; `displayed`
recomposes, from that run's --raw-frames-out and --features-out files, its event list and its flags,
every frame the view displayed, through the stage methods of RayTracer.  The state machine below is the
header's, event by event, and the only copy the tests have: every view test recomposes through it.  The
stages are the library's, so this pins how the view composes them, not what they compute (their own
tests do that against numpy restatements)."""
from __future__ import annotations

import json
import subprocess
import tempfile
from dataclasses import dataclass, replace
from pathlib import Path
from typing import NamedTuple

import numpy as np

from conftest import ROOT

F = np.float32
TARGET = (0.0, -4.0, 0.0)  # the view orbits it, whatever camera the application set
# rt_render's per-display outputs: their flags, and the element type of those that are arrays
OUTPUTS = {"shown": ("--frames-out", F), "raw": ("--raw-frames-out", F), "feat": ("--features-out", F),
           "f8": ("--frames8-out", np.uint32), "elog": ("--exposure-log", None), "ppm": ("--ppm", None)}


def run_view(tmp, args, outputs=("shown", "raw", "feat"), width=64, height=48) -> dict:
    """One `rt_render --width --height` run with `args`, its files in a directory of their own under
    `tmp`: the requested outputs by name (arrays; "elog" and "ppm" as paths) and, as "lines", the JSON
    lines it printed."""
    out = Path(tempfile.mkdtemp(dir=tmp))
    files = {k: out / k for k in outputs}
    cmd = [str(ROOT / "pathtracer.cl_amd" / "rt_render"), "--width", str(width), "--height", str(height), *args]
    for k, f in files.items():
        cmd += [OUTPUTS[k][0], str(f)]
    r = subprocess.run(cmd, check=True, timeout=120, capture_output=True, text=True)
    run = {k: np.fromfile(f, OUTPUTS[k][1]) if OUTPUTS[k][1] else f for k, f in files.items()}
    run["lines"] = [json.loads(l) for l in r.stdout.splitlines()]
    return run


@dataclass(frozen=True)
class Flags:
    """The display flags of rt_render with their optional values (the CLI's defaults)."""
    denoise: bool = False
    iterations: int = 5
    temporal: bool = False
    max_history: float = 32.0
    variance_guided: bool = False
    sigma_lum: float = 4.0
    motion_carry: bool = False
    motion_max_history: float = 8.0
    history_trust: bool = False
    tolerance: float = 1.5
    sphere_carry: bool = False
    sphere_max_history: float = 8.0

    def cli(self) -> list[str]:
        """The flags as rt_render takes them: bare where the value is the default."""
        args = []
        for on, flag, field in ((self.denoise, "--denoise", "iterations"), (self.temporal, "--temporal", "max_history"),
                                (self.variance_guided, "--variance-guided", "sigma_lum"),
                                (self.motion_carry, "--motion-carry", "motion_max_history"),
                                (self.history_trust, "--history-trust", "tolerance"),
                                (self.sphere_carry, "--sphere-carry", "sphere_max_history")):
            if on:
                value = getattr(self, field)
                args += [flag] if value == getattr(Flags, field) else [flag, str(value)]
        return args

    def without(self, name: str) -> "Flags":
        """This set with one flag off, and with it the flags rt_render refuses without it."""
        off = {name: False}
        if name == "temporal":
            off.update(motion_carry=False, history_trust=False, sphere_carry=False)
        return replace(self, **off)


class _History:
    """A kept pair and a carried pair, each an RGBA frame and its plane of history lengths."""

    def __init__(self, px):
        self.kept, self.kept_len = np.zeros(4 * px, F), np.zeros(px, F)
        self.carried, self.carried_len = np.zeros(4 * px, F), np.zeros(px, F)


class Displayed(NamedTuple):
    frames: list  # every displayed frame, in order
    lengths: list  # beside each, the colour history's kept lengths (None without --temporal)


def displayed(rt, scenes, flags: Flags, events: str, raw: np.ndarray, feats: np.ndarray, width: int, height: int,
              mesh=None, poses=None, max_progression: int = 10000, spheres0=None) -> Displayed:
    """The frames `rt_render --events` displayed, in order.  `rt` is a RayTracer to run the stages on,
    `scenes` the package's scenes module, `raw` / `feats` the whole --raw-frames-out / --features-out
    files.  A mesh view (--mesh) with p events gives `mesh` = (verts, idx), the run's mesh, and `poses`,
    the --poses file as [K, n_verts, 3]; a sphere view (no --mesh) gives `spheres0`, the scene's
    SPHERE_DTYPE list before any o or e event.  The warps read the current pose and the current spheres
    from `rt`, which is left with the last ones set."""
    fl = flags
    w, h = width, height
    az, el = F(105.0), F(40.0)
    # a sphere view keeps the camera the application set (main.cpp's) until the first key press
    camera = dict(scenes.MAIN_CAMERA) if spheres0 is not None else None
    realloc, progression = True, 0
    feat_dirty, carry, have_hist, mom_valid, pose_pending = True, False, False, False, False
    spheres_pending, shown_valid, shown_spheres = False, False, None
    feat = hist_cam = colour = moments = mom = last_raw = pose_prev = None
    pose = None if mesh is None else np.asarray(mesh[0], F)
    if spheres0 is not None:
        cur_spheres = spheres0.copy()
        offsets = np.zeros((len(spheres0), 4), F)  # the o events so far, per sphere, summed in float32 as the CLI does
        light = np.zeros(3, F)  # the e events so far: the last sphere is the light
    taken = [0, 0]  # floats of raw / feats consumed
    shown, lengths = [], []

    def restart():
        nonlocal progression, carry
        progression, carry = 0, True

    def drop():
        nonlocal have_hist, pose_pending, spheres_pending, mom_valid
        have_hist = pose_pending = spheres_pending = mom_valid = False

    def trace():
        nonlocal feat, feat_dirty, carry, have_hist, mom_valid, pose_pending, spheres_pending, hist_cam, colour, moments, mom
        nonlocal last_raw, shown_valid, shown_spheres
        px = w * h
        cur = np.ascontiguousarray(raw[taken[0]:taken[0] + 4 * px])
        feat_now = np.ascontiguousarray(feats[taken[1]:taken[1] + 8 * px])
        assert cur.size == 4 * px and feat_now.size == 8 * px, "the run displayed fewer frames than its events say"
        taken[0] += 4 * px
        taken[1] += 8 * px
        n = max(progression, 1)
        if fl.variance_guided:
            n_mom = n if mom_valid else 1
            new = np.zeros(4 * px, F)
            rt.momentsAccumulate(last_raw if n_mom > 1 else None, cur, n_mom, mom if n_mom > 1 else None, new, w, h)
            mom, mom_valid = new, True
        hist_feat = feat  # the features the kept frame was displayed with
        if fl.denoise or fl.temporal or fl.variance_guided:
            if feat_dirty:  # rendered again: with --temporal the old ones are kept, and the history is carried
                if fl.temporal:
                    carry = True
                feat, feat_dirty = feat_now, False
            else:  # the view's features are those the CLI renders beside every displayed frame
                assert np.array_equal(feat.view(np.uint32), feat_now.view(np.uint32))
        disp, disp_mom, length = cur, mom, None
        if fl.temporal:
            active = [(colour, cur)] + ([(moments, mom)] if fl.variance_guided else [])
            cam = scenes.camera_spherical(w, **(camera or dict(target=TARGET, elevation=float(el), azimuth=float(az), distance=5.0)))
            judged = fl.history_trust and have_hist
            if not have_hist:
                for hs, _ in active:
                    hs.carried[:], hs.carried_len[:] = 0.0, 0.0
            elif carry:
                cur_feat, cap = feat, fl.max_history
                if pose_pending:  # the mesh has moved since: the taps are sought where the material was
                    rt.setMesh(*mesh)
                    rt.updateMesh(pose)
                    cur_feat = np.zeros_like(feat)
                    rt.warpFeatures(feat, pose_prev, cur_feat, w, h)
                    cap = min(cap, fl.motion_max_history)
                if spheres_pending:  # spheres have moved since: the taps are sought where each sphere stood
                    rt.setSpheres(cur_spheres)
                    warped = np.zeros_like(feat)
                    rt.warpFeaturesSpheres(cur_feat, shown_spheres, warped, w, h)
                    cur_feat, cap = warped, min(cap, fl.sphere_max_history)
                for hs, _ in active:  # the moments with the colour's lengths
                    rt.reproject(hs.kept, colour.kept_len, hist_feat, hist_cam, cur_feat, hs.carried, hs.carried_len, w, h,
                                 max_history=cap)
            pose_pending = spheres_pending = carry = False
            trusted = None
            if judged:
                trusted = np.zeros(px, F)
                rt.historyTrust(colour.carried, colour.carried_len, cur, n, feat, trusted, w, h, tolerance=fl.tolerance)
            for hs, src in active:
                hs.kept, hs.kept_len = np.zeros(4 * px, F), np.zeros(px, F)
                rt.temporalMerge(hs.carried, trusted if judged else hs.carried_len, src, n, hs.kept, hs.kept_len, w, h,
                                 max_history=fl.max_history)
                for mine, colours in ((hs.carried_len, colour.carried_len), (hs.kept_len, colour.kept_len)):
                    assert np.array_equal(mine.view(np.uint32), colours.view(np.uint32))  # one length for both histories
            hist_cam, have_hist = cam, True
            disp, disp_mom, length = colour.kept, moments.kept, colour.kept_len
        elif fl.variance_guided:
            length = np.full(px, n, F)
        if fl.variance_guided:  # in place of --denoise's filter, whether that is given or not
            var, out = np.zeros(px, F), np.zeros(4 * px, F)
            rt.variance(disp, disp_mom, length, feat, var, w, h)
            rt.denoiseVar(disp, var, feat, out, None, w, h, sigma_lum=fl.sigma_lum)
            disp = out
        elif fl.denoise:
            out = np.zeros(4 * px, F)
            rt.denoise(disp, feat, out, w, h, iterations=fl.iterations)
            disp = out
        last_raw = cur
        shown.append(disp)
        lengths.append(colour.kept_len if fl.temporal else None)
        if fl.sphere_carry and spheres0 is not None:  # the spheres this frame was displayed with
            shown_spheres, shown_valid = cur_spheres.copy(), True

    for ev in filter(None, events.split(",")):
        kind, args = ev[0], ev.split(":")[1:]
        if ev == "d":
            if realloc:  # allocate(): everything of the old size goes, the pose snapshot included
                colour, moments = _History(w * h), _History(w * h)
                feat = mom = last_raw = None
                feat_dirty = True
                drop()
                progression, realloc = 0, False
                trace()
            elif progression < max_progression:
                progression += 1
                trace()
        elif ev in ("l", "r", "u", "n") or kind == "m":
            d_az, d_el = {"l": (3, 0), "r": (-3, 0), "u": (0, 3), "n": (0, -3)}[ev] if kind != "m" else map(int, args)
            az = np.fmod(F(az + F(d_az)), F(360.0))
            el = np.fmax(np.fmin(F(el + F(d_el)), F(90.0)), F(10.0))
            camera = None  # the orbit camera from here on
            feat_dirty = True
            restart()
        elif kind == "s":
            w, h = int(args[0]), int(args[1])
            realloc = True
        elif kind in ("e", "o"):  # sceneChanged: the light moved by DX:DY:DZ, or sphere I by DX:DY:DZ[:DR]
            if spheres0 is not None:  # (in a mesh view the spheres are lights only, and nothing reads them here)
                if kind == "e":
                    light += np.array([float(a) for a in args], F)
                else:
                    offsets[int(args[0])] += np.array([float(a) for a in args[1:]] + [0.0] * (5 - len(args)), F)
                cur_spheres = spheres0.copy()
                cur_spheres["center"][-1] = spheres0["center"][-1] + light
                for j in np.flatnonzero((offsets != 0).any(axis=1)):  # an untouched sphere keeps its bits
                    cur_spheres["center"][j] = cur_spheres["center"][j] + offsets[j, :3]
                    cur_spheres["radius"][j] = cur_spheres["radius"][j] + offsets[j, 3]
            carry_spheres = fl.sphere_carry and fl.temporal and have_hist and shown_valid and not realloc
            feat_dirty = True
            if carry_spheres:  # the oldest list since the last display: shown_spheres changes at displays only
                spheres_pending = True
            elif not fl.history_trust:
                drop()
            restart()
            if not carry_spheres and not fl.history_trust:
                carry = False
        elif kind == "p":  # updateMesh
            carry_motion = fl.motion_carry and fl.temporal and have_hist and not realloc
            if carry_motion and not pose_pending:  # the oldest pose since the last display
                pose_prev, pose_pending = pose, True
            pose = np.ascontiguousarray(poses[int(args[0])], F)
            feat_dirty = True
            if not carry_motion:
                drop()
            restart()
            if not carry_motion:
                carry = False
        else:
            raise ValueError(f"event {ev!r}")
    assert taken == [raw.size, feats.size], "the run displayed more frames than its events say"
    return Displayed(shown, lengths)
