"""ProgressiveViewHIP's display chain, restated once for every flag set rt_render accepts (DESIGN.md
§4.8): from a run's --raw-frames-out and --features-out files, its event list and its flags, every
frame the view displayed, recomposed through the stage methods of RayTracer.  The state machine below
is the header's, event by event; the stages are the library's, so this pins how the view composes
them, not what they compute (their own tests do that against numpy restatements)."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

F = np.float32
TARGET = (0.0, -4.0, 0.0)  # the view orbits it, whatever camera the application set


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

    def cli(self) -> list[str]:
        """The flags as rt_render takes them: bare where the value is the default."""
        args = []
        for on, flag, field in ((self.denoise, "--denoise", "iterations"), (self.temporal, "--temporal", "max_history"),
                                (self.variance_guided, "--variance-guided", "sigma_lum"),
                                (self.motion_carry, "--motion-carry", "motion_max_history"),
                                (self.history_trust, "--history-trust", "tolerance")):
            if on:
                value = getattr(self, field)
                args += [flag] if value == getattr(Flags, field) else [flag, str(value)]
        return args

    def without(self, name: str) -> "Flags":
        """This set with one flag off, and with it the flags rt_render refuses without it."""
        off = {name: False}
        if name == "temporal":
            off.update(motion_carry=False, history_trust=False)
        return replace(self, **off)


class _History:
    """A kept pair and a carried pair, each an RGBA frame and its plane of history lengths."""

    def __init__(self, px):
        self.kept, self.kept_len = np.zeros(4 * px, F), np.zeros(px, F)
        self.carried, self.carried_len = np.zeros(4 * px, F), np.zeros(px, F)


def displayed(rt, scenes, flags: Flags, events: str, raw: np.ndarray, feats: np.ndarray, width: int, height: int,
              mesh=None, poses=None, max_progression: int = 10000) -> list[np.ndarray]:
    """The frames `rt_render --events` displayed, in order.  `rt` is a RayTracer to run the stages on
    (with `mesh` = (verts, idx), the run's mesh, set if there are p events: the warp reads the current
    pose from it), `scenes` the package's scenes module, `raw` / `feats` the whole --raw-frames-out /
    --features-out files, `poses` the --poses file as [K, n_verts, 3]."""
    fl = flags
    w, h = width, height
    az, el = F(105.0), F(40.0)
    realloc, progression = True, 0
    feat_dirty, carry, have_hist, mom_valid, pose_pending = True, False, False, False, False
    feat = hist_cam = colour = moments = mom = last_raw = pose_prev = None
    pose = None if mesh is None else np.asarray(mesh[0], F)
    taken = [0, 0]  # floats of raw / feats consumed
    shown = []

    def restart():
        nonlocal progression, carry
        progression, carry = 0, True

    def drop(moments_too=True):
        nonlocal have_hist, pose_pending, mom_valid
        have_hist = pose_pending = False
        if moments_too:
            mom_valid = False

    def trace():
        nonlocal feat, feat_dirty, carry, have_hist, mom_valid, pose_pending, hist_cam, colour, moments, mom, last_raw
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
            cam = scenes.camera_spherical(w, target=TARGET, elevation=float(el), azimuth=float(az), distance=5.0)
            judged = fl.history_trust and have_hist
            if not have_hist:
                for hs, _ in active:
                    hs.carried[:], hs.carried_len[:] = 0.0, 0.0
            elif carry:
                cur_feat, cap = feat, fl.max_history
                if pose_pending:
                    rt.setMesh(*mesh)
                    rt.updateMesh(pose)
                    cur_feat = np.zeros_like(feat)
                    rt.warpFeatures(feat, pose_prev, cur_feat, w, h)
                    cap = min(fl.max_history, fl.motion_max_history)
                for hs, _ in active:  # the moments with the colour's lengths
                    rt.reproject(hs.kept, colour.kept_len, hist_feat, hist_cam, cur_feat, hs.carried, hs.carried_len, w, h,
                                 max_history=cap)
            pose_pending = carry = False
            trusted = None
            if judged:
                trusted = np.zeros(px, F)
                rt.historyTrust(colour.carried, colour.carried_len, cur, n, feat, trusted, w, h, tolerance=fl.tolerance)
            for hs, src in active:
                hs.kept, hs.kept_len = np.zeros(4 * px, F), np.zeros(px, F)
                rt.temporalMerge(hs.carried, trusted if judged else hs.carried_len, src, n, hs.kept, hs.kept_len, w, h,
                                 max_history=fl.max_history)
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
            feat_dirty = True
            restart()
        elif kind == "s":
            w, h = int(args[0]), int(args[1])
            realloc = True
        elif kind == "e":  # sceneChanged
            feat_dirty = True
            if not fl.history_trust:
                drop()
            restart()
            if not fl.history_trust:
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
    return shown
