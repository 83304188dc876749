"""``BatchedEnv`` — one shard of N in-process envs on one MI355X, over the C ABI of ``include/trsim.h``.

It is the batched form of what the reference's per-car ``GymInterface`` does for one car
(``TritonRacerSim/components/gyminterface.py:49-104``): controls in, ``(image, x, y, z, speed, cte)``
out, plus ``LocationTracker``'s index (``components/track_data_process.py:89-107``).  All outputs stay
device-resident; host copies happen only on request (``fetch``).
"""
import ctypes as C
import json
import os

import numpy as np

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
TRACK_DIR = os.path.join(_HERE, "track_data")

_FIELD_DTYPES = {
    "img": np.uint8, "pos_x": np.float32, "pos_y": np.float32, "pos_z": np.float32, "speed": np.float32,
    "cte": np.float32, "yaw": np.float32, "vel": np.float32, "seg_idx": np.int32, "ep_return": np.float32,
    "last_return": np.float32, "ep_len": np.int32, "done": np.uint8, "map": np.uint32, "rowtab": np.float32,
    "palette": np.uint32, "tangent": np.float32, "steer_filt": np.float32, "stats": np.uint64, "depth": np.float32, "rowdepth": np.float32,
    "ctl_steer": np.float32, "ctl_thr": np.float32, "ctl_brk": np.float32, "dpitch": np.float32,
    "lens_table": np.float32, "lens_palette": np.uint32,
}


def resolve_track(track):
    """Accepts an ``(n,3)`` array, a JSON path, or a scene / file name as the reference configs use them
    (``scene_name`` ``core/config.py:94``, ``track_data_file`` ``core/config.py:101``)."""
    if isinstance(track, (list, tuple, np.ndarray)):
        pts = np.asarray(track, dtype=np.float64)
    else:
        name = str(track)
        candidates = [name, os.path.join(TRACK_DIR, name), os.path.join(TRACK_DIR, os.path.basename(name)),
                      os.path.join(TRACK_DIR, os.path.splitext(os.path.basename(name))[0] + ".json")]
        for c in candidates:
            if os.path.isfile(c):
                with open(c) as f:
                    pts = np.asarray(json.load(f), dtype=np.float64)
                break
        else:
            raise FileNotFoundError(f"no track data for {track!r} (looked in {TRACK_DIR})")
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 2:
        raise ValueError("track must be an (n>=2, 3) array of [x, y, z]")
    return np.ascontiguousarray(pts)


class _DevicePtr:
    """Zero-copy view of a device array for torch / cupy (``__cuda_array_interface__``).  The producing work has been
    ordered before the view is handed out (``BatchedEnv.device_array``: a host synchronisation, or a wait queued on the
    consumer's stream), so the interface carries no stream of its own."""

    def __init__(self, ptr, shape, dtype, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (int(ptr), False), "version": 2, "strides": None,
        }


def device_ptr(x):
    """Device address of a zero-copy handle: anything with ``__cuda_array_interface__`` (this module's handles, torch / cupy
    arrays), or an integer; ``None`` / ``0`` stay ``None``."""
    if x is None:
        return None
    if hasattr(x, "__cuda_array_interface__"):
        return int(x.__cuda_array_interface__["data"][0]) or None
    return int(x) or None


def is_device_array(x):
    return hasattr(x, "__cuda_array_interface__")


# handle-owned scratch slots (trs_scratch) the device-resident parts use for the values that travel between them
SLOT_AI = (0, 1, 2)            # 'ai/steering', 'ai/throttle', 'ai/breaking'    (HipKerasPilot)
SLOT_MODE = 3                  # 'usr/mode' as uint8 codes                         (BatchedControlMultiplexer, HipKerasPilot)
SLOT_USR = (4, 5, 6)           # 'usr/steering', 'usr/throttle', 'usr/breaking'   (uploaded joystick values)
SLOT_MUX = (7, 8, 9)           # 'mux/steering', 'mux/throttle', 'mux/breaking'   (BatchedControlMultiplexer)
SLOT_PILOT_IN = (10, 11)       # 'gym/speed', 'loc/segment' that reached HipKerasPilot as HOST values beside a device frame
SLOT_JPEG_IN = 12              # host frames handed to BatchedEnv.encode_jpeg                        (uploaded before the encoder reads them)
SLOT_EXPERT = (13, 14, 15)     # 'usr/steering', 'usr/throttle', 'usr/breaking' of the scripted expert (BatchedEnv.expert_act, HipScriptedDriver)
SLOT_COLLECT = (16, 17)        # the frames and rows of BatchedEnv.collect


def _stream_ptr(stream):
    """A HIP stream as an integer: accepts ``torch.cuda.Stream`` (``.cuda_stream``), cupy streams (``.ptr``) or the raw
    pointer value; ``0`` is the legacy default stream."""
    for attr in ("cuda_stream", "ptr"):
        if hasattr(stream, attr):
            return int(getattr(stream, attr))
    return int(stream)


def lighting_array(params, bias=None, n=None):
    """Scene-lighting parameters as the library takes them: float32 ``[n, 8]`` = ``{gR, gG, gB, 0, bR, bG, bB, 0}`` per env, from an
    ``[n, 8]`` array, or from gain ``[n, 3]`` and bias ``[n, 3]``."""
    if bias is not None:
        g, b = np.asarray(params, np.float32), np.asarray(bias, np.float32)
        if g.ndim != 2 or g.shape[1] != 3 or b.shape != g.shape:
            raise ValueError("gain and bias must both be [n_envs, 3]")
        out = np.zeros((g.shape[0], 8), np.float32)
        out[:, 0:3], out[:, 4:7] = g, b
    else:
        out = np.ascontiguousarray(params, np.float32)
        if out.ndim != 2 or out.shape[1] != 8:
            raise ValueError("lighting parameters must be [n_envs, 8] (or gain and bias [n_envs, 3] each)")
    if n is not None and out.shape[0] != n:
        raise ValueError(f"lighting parameters for {out.shape[0]} envs, the env has {n}")
    return np.ascontiguousarray(out)


def lighting_params(n, seed=0, gain=(0.6, 1.4), bias=(-30.0, 30.0), per_channel=True):
    """Random scene lighting for domain randomisation: float32 ``[n, 8]`` with gains uniform in ``gain`` and biases uniform in ``bias``
    (one draw per env and channel; ``per_channel=False``: one gain and one bias per env, the same on R, G and B), from ``seed``."""
    rng = np.random.default_rng(seed)
    k = 3 if per_channel else 1
    g = np.broadcast_to(rng.uniform(gain[0], gain[1], (n, k)), (n, 3))
    b = np.broadcast_to(rng.uniform(bias[0], bias[1], (n, k)), (n, 3))
    return lighting_array(g.astype(np.float32), b.astype(np.float32))


def corner_speed_profile(track_xyz, a_lat, v_max, span=4, ahead=12):
    """ONE possible speed profile for ``BatchedEnv.set_expert(profile=...)``: slow down for the corners ahead.  Per raw track point ``i`` of the closed
    centre line (x, z; indices wrap): the turn between the chords ``P[i-span] -> P[i]`` and ``P[i] -> P[i+span]`` over their mean length is the
    curvature, ``v_i = min(v_max, sqrt(a_lat / curvature))`` the speed a lateral acceleration ``a_lat`` allows there, and the profile is the minimum
    of ``v`` over points ``i .. i + ahead``.  float32 ``[n_points]``.  The library holds no curvature model: any array of that shape will do."""
    pts = np.asarray(track_xyz, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("track must be an (n, 3) array of [x, y, z]")
    span, ahead = int(span), int(ahead)
    if span < 1 or ahead < 0 or not a_lat > 0 or not v_max > 0:
        raise ValueError("span >= 1, ahead >= 0, a_lat > 0 and v_max > 0 are required")
    xz = pts[:, [0, 2]]
    back, fwd = xz - np.roll(xz, span, axis=0), np.roll(xz, -span, axis=0) - xz
    turn = np.arctan2(fwd[:, 0], fwd[:, 1]) - np.arctan2(back[:, 0], back[:, 1])
    turn = np.abs((turn + np.pi) % (2 * np.pi) - np.pi)
    dist = 0.5 * (np.hypot(back[:, 0], back[:, 1]) + np.hypot(fwd[:, 0], fwd[:, 1]))
    curv = np.where(dist > 1e-9, turn / np.maximum(dist, 1e-9), 0.0)
    v = np.minimum(float(v_max), np.sqrt(float(a_lat) / np.maximum(curv, 1e-12)))
    out = v.copy()
    for k in range(1, ahead + 1):
        out = np.minimum(out, np.roll(v, -k))
    return np.ascontiguousarray(out, dtype=np.float32)


class JpegFrames:
    """The JPEG files of one ``BatchedEnv.encode_jpeg`` call: ``len()``, ``[i] -> bytes``, iteration; ``.blob`` (uint8, the files that fitted back to
    back), ``.offsets`` (int64[n + 1] into ``.blob``) and ``.lengths`` (int32[n]; negative: the file did not fit and was encoded on the host)."""

    def __init__(self, blob, offsets, lengths, late=None):
        self.blob, self.offsets, self.lengths = blob, offsets, lengths
        self._late = late or {}

    def __len__(self):
        return int(self.lengths.shape[0])

    def __getitem__(self, i):
        n = len(self)
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(n))]
        i = int(i)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        if i in self._late:
            return self._late[i]
        return self.blob[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()


class BatchedEnv:
    def __init__(self, n_envs=1, track="generated_track", device=0, img_h=120, img_w=160, render=True,
                 auto_reset=False, env_id_base=0, seed=None, depth=False, camera=None, _api=None, **overrides):
        # `_api` exists for tests only (they pass the oracle's function table to diff both through one
        # wrapper); the product path always binds the HIP library and raises if it is not built.
        self.api = _api if _api is not None else _ffi.load_hip_library()
        cfg = _ffi.TrsConfig()
        self.api.default_config(C.byref(cfg))
        cfg.n_envs, cfg.env_id_base, cfg.img_h, cfg.img_w = int(n_envs), int(env_id_base), int(img_h), int(img_w)
        cfg.render, cfg.auto_reset, cfg.depth = int(bool(render)), int(bool(auto_reset)), int(bool(depth))
        if seed is not None:
            cfg.seed = int(seed)
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown env parameter {k!r}")
            setattr(cfg, k, v)
        self.cfg = cfg
        self.n, self.H, self.W = int(n_envs), int(img_h), int(img_w)
        self.device = int(device)
        self._h = C.c_void_p()
        self.api.check(self.api.create(C.byref(cfg), self.device, C.byref(self._h)), "create")
        self.track = None
        self.map_info = None
        if track is not None:
            self.load_track(track)
        if camera is not None:          # a dict of set_camera's keywords, or a (fish_eye_x, fish_eye_y, offset_x) triple
            if isinstance(camera, dict):
                self.set_camera(**camera)
            else:
                self.set_camera(*camera)

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.api.destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_track(self, track):
        pts = resolve_track(track)
        self.api.check(self.api.load_track(self._h, pts.ctypes.data, int(pts.shape[0])), "load_track")
        self.track = pts
        mi = _ffi.TrsMapInfo()
        self.api.check(self.api.map_info_get(self._h, C.byref(mi)), "map_info_get")
        self.map_info = mi

    @property
    def n_points(self):
        return 0 if self.track is None else int(self.track.shape[0])

    # -- stepping ----------------------------------------------------------------------------
    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.n,):
            raise ValueError("mask must have shape (n_envs,)")
        self.api.check(self.api.reset(self._h, None if m is None else m.ctypes.data), "reset")

    def _ctl(self, a, name, optional=False):
        if a is None:
            if optional:
                return None
            raise ValueError(f"{name} is required")
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), (self.n,)))
        return arr

    def step(self, steering, throttle, brake=None, reset=None, n_steps=1):
        """Host-array controls (numpy / scalars).  Asynchronous; ``fetch`` synchronises."""
        st, th, br = self._ctl(steering, "steering"), self._ctl(throttle, "throttle"), self._ctl(brake, "brake", True)
        rs = None if reset is None else np.ascontiguousarray(np.broadcast_to(np.asarray(reset).astype(bool), (self.n,)), dtype=np.uint8)
        self.api.check(self.api.step_host(self._h, st.ctypes.data, th.ctypes.data, None if br is None else br.ctypes.data,
                                          None if rs is None else rs.ctypes.data, int(n_steps)), "step_host")

    def step_device(self, d_steering, d_throttle, d_brake=0, d_reset=0, n_steps=1, stream=None):
        """Raw device pointers (ints), e.g. ``tensor.data_ptr()`` of float32 / uint8 CUDA tensors.  The env works on its own
        stream: pass ``stream=`` (the stream that PRODUCES the control tensors, e.g. ``torch.cuda.current_stream()``) and the
        step is ordered behind that stream's work (``trs_stream_wait_external``: an event wait, no host synchronisation in
        launch mode); without it the caller must have synchronised the producer."""
        if stream is not None:
            self.api.check(self.api.stream_wait_external(self._h, _stream_ptr(stream) or None), "stream_wait_external")
        self.api.check(self.api.step(self._h, int(d_steering), int(d_throttle), int(d_brake) or None, int(d_reset) or None,
                                     int(n_steps)), "step")

    def step_device_wait(self, d_steering, d_throttle, d_brake=0, d_reset=0, n_steps=1):
        """``step_device`` and ``sync`` in one call (``trs_step_wait``): the lock-step tick — post the controls, return when the
        frame and the telemetry are complete — with one FFI crossing."""
        self.api.check(self.api.step_wait(self._h, int(d_steering), int(d_throttle), int(d_brake) or None, int(d_reset) or None,
                                          int(n_steps)), "step_wait")

    def step_sequence(self, steering, throttle, brake=None, reset=None, steps_per_launch=8):
        """Open-loop action sequences: ``steering`` / ``throttle`` / ``brake`` are ``[n_steps, n_envs]`` host arrays, one
        control set per step (``trs_step_sequence_host``); the call runs ``steps_per_launch`` steps per kernel launch."""
        st = np.ascontiguousarray(steering, dtype=np.float32)
        k = st.shape[0]
        f = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), (k, self.n)))
        st, th = f(st), f(throttle)
        br = None if brake is None else f(brake)
        rs = None if reset is None else np.ascontiguousarray(np.broadcast_to(np.asarray(reset, dtype=np.uint8), (self.n,)))
        self.api.check(self.api.step_sequence_host(self._h, st.ctypes.data, th.ctypes.data, None if br is None else br.ctypes.data,
                                                   None if rs is None else rs.ctypes.data, int(k), int(steps_per_launch)), "step_sequence_host")

    def step_sequence_device(self, d_steering, d_throttle, d_brake=0, d_reset=0, n_steps=1, steps_per_launch=8):
        """Same with raw device pointers to ``float32[n_steps, n_envs]`` arrays."""
        self.api.check(self.api.step_sequence(self._h, int(d_steering), int(d_throttle), int(d_brake) or None, int(d_reset) or None,
                                              int(n_steps), int(steps_per_launch)), "step_sequence")

    def step_synthetic(self, n_steps=1, steps_per_launch=1):
        self.api.check(self.api.step_synthetic(self._h, int(n_steps), int(steps_per_launch)), "step_synthetic")

    def set_step_mode(self, resident=True, idle_us=0):
        """``resident=True``: a worker kernel stays on the GPU and every ``step*`` call only posts its controls
        (``trs_set_step_mode``: no launch, no kernel boundary, no table re-staging per step); ``False``: one launch per call."""
        self.api.check(self.api.set_step_mode(self._h, 1 if resident else 0, int(idle_us)), "set_step_mode")

    def sync(self):
        self.api.check(self.api.sync(self._h), "sync")

    def step_mode(self):
        """``("resident" | "launch", fell_back)`` (``trs_get_step_mode``).  ``fell_back``: resident mode was selected and the library went back to
        launches by itself because the GPU is shared with another process's resident worker (``include/trsim.h``)."""
        mode, fb = C.c_int(0), C.c_int(0)
        self.api.check(self.api.get_step_mode(self._h, C.byref(mode), C.byref(fb)), "get_step_mode")
        return ("resident" if mode.value == 1 else "launch"), bool(fb.value)

    def quiesce(self):
        """Resident mode: the worker kernel leaves the GPU (posted steps complete first); the next step starts a new one
        (``trs_quiesce``).  Call before work of another stream that needs the CUs the worker occupies (collectives)."""
        self.api.check(self.api.quiesce(self._h), "quiesce")

    # -- outputs -----------------------------------------------------------------------------
    def _shape(self, name):
        mi = self.map_info
        return {
            "img": (self.n, self.H, self.W, 3), "map": (mi.map_h, mi.map_words) if mi else None,
            "rowtab": (self.H, 2), "palette": (self.H, 4), "tangent": (self.n_points, 2), "stats": (64,), "depth": (self.n, self.H, self.W), "rowdepth": (self.H,),
            "dpitch": (self.n_points,), "lens_table": (self.H, self.W, 4), "lens_palette": (513, 4),
        }.get(name, (self.n,))

    def fetch(self, name):
        """Synchronising device→host copy of one output field as a fresh numpy array."""
        shape = self._shape(name)
        out = np.empty(shape, dtype=_FIELD_DTYPES[name])
        self.api.check(self.api.copy_to_host(self._h, _ffi.FIELDS[name], out.ctypes.data, out.nbytes), f"copy_to_host({name})")
        return out

    def fetch_outputs(self, image=True):
        """``(img, x, y, z, speed, cte, seg_idx, done)`` of all envs as fresh numpy arrays in one synchronisation
        (``trs_fetch_outputs``): what ``GymInterface.step`` returns plus the tracker index and the done flag."""
        n = self.n
        img = np.empty((n, self.H, self.W, 3), np.uint8) if image else None
        f = [np.empty(n, np.float32) for _ in range(5)]
        seg, done = np.empty(n, np.int32), np.empty(n, np.uint8)
        self.api.check(self.api.fetch_outputs(self._h, img.ctypes.data if image else None, *[a.ctypes.data for a in f],
                                              seg.ctypes.data, done.ctypes.data), "fetch_outputs")
        return (img, *f, seg, done)

    def state_view(self):
        sv = _ffi.TrsStateView()
        self.api.check(self.api.get_state(self._h, C.byref(sv)), "get_state")
        return sv

    def device_array(self, name, stream=None, sync=True):
        """Zero-copy handle (``__cuda_array_interface__``) on a device-resident output; use
        ``torch.as_tensor(env.device_array('ep_return'), device='cuda')``.  The env's steps run on the env's own stream, so
        the view is ordered first: with ``stream=`` (the CONSUMER's stream) that stream is made to wait for the env's work
        queued so far (``trs_stream_signal_external``), otherwise the host waits (``sync=False`` skips even that: the caller
        orders).  ``'img'`` / ``'depth'`` alternate between two buffers: the frame of step s is overwritten by step s + 2.
        The frame buffers are READ-ONLY for the consumer: rows that do not depend on the pose (sky, ground beyond the far plane) are
        written once per buffer and palette, later steps store only the rows that see the track — bytes written into a view would
        show up in those rows two steps later.  Clone a frame before changing it."""
        if stream is not None:
            self.api.check(self.api.stream_signal_external(self._h, _stream_ptr(stream) or None), "stream_signal_external")
        elif sync:
            self.sync()
        sv = self.state_view()
        ptr = getattr(sv, name)
        if not ptr:
            raise RuntimeError(f"{name} is not available")
        return _DevicePtr(ptr, self._shape(name), _FIELD_DTYPES[name], self)

    def set_pose(self, x=None, y=None, z=None, yaw=None, v=None):
        arrs = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), (self.n,))) for a in (x, y, z, yaw, v)]
        self.api.check(self.api.set_pose(self._h, *[None if a is None else a.ctypes.data for a in arrs]), "set_pose")

    def locate(self, points):
        """Batched ``LocationTracker.__find_closest`` (``track_data_process.py:89-101``) → int32 indices."""
        q = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        out = np.empty(q.shape[0], dtype=np.int32)
        self.api.check(self.api.locate(self._h, q.ctypes.data, int(q.shape[0]), out.ctypes.data), "locate")
        return out

    def segment(self, idx, min_map=0.0, max_map=10.0):
        """``LocationTracker.__map`` (``track_data_process.py:106-107``): index → 'loc/segment' float."""
        return np.asarray(idx, dtype=np.float64) / float(self.n_points) * (max_map - min_map) + min_map

    # -- image path (ImgPreprocessing + pilot normalisation) ------------------------------------
    def pre_config(self, cfg=None):
        """``trs_pre_config`` from the reference's ``preprocessing_*`` keys (``core/config.py:15-28``)."""
        pc = _ffi.TrsPreConfig()
        self.api.default_pre_config(C.byref(pc))
        cfg = cfg or {}
        pc.dynamic_brightness = int(bool(cfg.get("preprocessing_dynamic_brightness_enabled", False)))
        pc.brightness_baseline = float(cfg.get("preprocessing_brightness_baseline", 550))
        pc.contrast_ratio = float(cfg.get("preprocessing_contrast_enhancement_ratio", 1.0))
        pc.contrast_offset = float(cfg.get("preprocessing_contrast_enhancement_offset", 125))
        pc.color_filter_enabled = int(bool(cfg.get("preprocessing_color_filter_enabled", False)))
        pc.edge_detection_enabled = int(bool(cfg.get("preprocessing_edge_detection_enabled", False)))
        pc.edge_threshold_a = int(cfg.get("preprocessing_edge_detection_threshold_a", 60))
        pc.edge_threshold_b = int(cfg.get("preprocessing_edge_detection_threshold_b", 100))
        pc.edge_dst_channel = int(cfg.get("preprocessing_edge_detection_destination_channel", 2))
        if "preprocessing_color_filter_hsvs" in cfg:
            bounds = cfg["preprocessing_color_filter_hsvs"]
            chans = cfg.get("preprocessing_color_filter_destination_channels", list(range(len(bounds))))
            if len(bounds) > 4 or len(chans) != len(bounds):
                raise ValueError("at most 4 colour filters, one destination channel each")
            pc.n_filters = len(bounds)
            for f, (lo, hi) in enumerate(bounds):
                for k in range(3):
                    pc.hsv_lo[f][k], pc.hsv_hi[f][k] = int(min(lo[k], 255)), int(min(hi[k], 255))
                pc.dst_channel[f] = int(chans[f])
        return pc

    def preprocess_host(self, frames, cfg=None):
        """``ImgPreprocessing.__process`` (no Canny) for host frames ``uint8[n,H,W,3]`` -> fresh ndarray."""
        src = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, self.H, self.W, 3)
        dst = np.empty_like(src)
        pc = cfg if isinstance(cfg, _ffi.TrsPreConfig) else self.pre_config(cfg)
        self.api.check(self.api.preprocess_host(self._h, C.byref(pc), src.ctypes.data, dst.ctypes.data, int(src.shape[0])), "preprocess_host")
        return dst

    def preprocess_latest(self, cfg=None):
        """Process the env's latest frames on the device; returns a zero-copy handle on ``uint8[N,H,W,3]``."""
        pc = cfg if isinstance(cfg, _ffi.TrsPreConfig) else self.pre_config(cfg)
        out = C.c_void_p()
        self.api.check(self.api.preprocess(self._h, C.byref(pc), None, None, self.n, C.byref(out)), "preprocess")
        return _DevicePtr(out.value, (self.n, self.H, self.W, 3), np.uint8, self)

    def set_camera(self, fish_eye_x=0.0, fish_eye_y=0.0, offset_x=0.0):
        """The lens camera (``trs_set_camera``; include/trsim_spec.h, "lens camera"): the ``fish_eye_x`` / ``fish_eye_y`` barrel strengths
        (each in [0, 2]) and the lateral camera mount ``offset_x`` (world units, + = right of the heading, within +-2) of the reference's
        gym_config.  ``set_camera(None)`` or all zero: the pinhole camera, byte for byte.  Flat tracks only; takes effect from the next step."""
        if not getattr(self.api, "has_lens", False):
            raise RuntimeError("this library has no lens camera (trs_set_camera)")
        if fish_eye_x is None:
            self.api.check(self.api.set_camera(self._h, None), "set_camera")
            return
        cam = _ffi.TrsCamera()
        self.api.default_camera(C.byref(cam))
        cam.fish_eye_x, cam.fish_eye_y, cam.offset_x = float(fish_eye_x), float(fish_eye_y), float(offset_x)
        self.api.check(self.api.set_camera(self._h, C.byref(cam)), "set_camera")

    def camera(self):
        """``(fish_eye_x, fish_eye_y, offset_x)`` of the camera that is set (``trs_get_camera``; all zero = the pinhole)."""
        cam = _ffi.TrsCamera()
        self.api.check(self.api.get_camera(self._h, C.byref(cam)), "get_camera")
        return cam.fish_eye_x, cam.fish_eye_y, cam.offset_x

    def set_lighting(self, params=None, bias=None):
        """Scene lighting per env (``trs_set_lighting``; include/trsim_spec.h, "scene lighting"): a colour gain and bias per env and channel on
        every rendered pixel, before any frame filter.  ``params``: ``None`` (unlit: frames byte for byte as before), a host array ``[n_envs, 8]``
        (``{gR, gG, gB, 0, bR, bG, bB, 0}`` per env), or gain ``[n_envs, 3]`` with ``bias=[n_envs, 3]``, which the library copies — or a device
        float32 ``[n_envs, 8]`` array (a torch CUDA tensor), registered zero-copy: the env keeps a reference, and values the caller rewrites
        between steps (ordered before the step, e.g. through ``step_device(..., stream=)``) take effect at the next step without a new call.
        Refused (``TRS_ERR_STATE``) without a camera and with a lens camera."""
        if not getattr(self.api, "has_lighting", False):
            raise RuntimeError("this library has no scene lighting (trs_set_lighting)")
        if params is None:
            self.api.check(self.api.set_lighting(self._h, None), "set_lighting")
            self._light_ref = None
            return
        if is_device_array(params):
            cai = params.__cuda_array_interface__
            if bias is not None:
                raise ValueError("a device array carries gain and bias together: float32 [n_envs, 8]")
            if tuple(cai["shape"]) != (self.n, 8) or np.dtype(cai["typestr"]) != np.float32 or cai.get("strides") not in (None, (32, 4)):
                raise ValueError(f"lighting parameters on the device must be a contiguous float32 [{self.n}, 8] array")
            self.api.check(self.api.set_lighting(self._h, device_ptr(params)), "set_lighting")
            self._light_ref = params
            return
        h = lighting_array(params, bias, self.n)
        self.api.check(self.api.set_lighting_host(self._h, h.ctypes.data_as(C.POINTER(C.c_float))), "set_lighting_host")
        self._light_ref = None

    # -- observation latency (trs_set_latency; include/trsim_spec.h, "observation latency") ----------------------------------
    _OBS_DTYPES = {"img": np.uint8, "depth": np.float32, "pos_x": np.float32, "pos_y": np.float32, "pos_z": np.float32, "speed": np.float32,
                   "cte": np.float32, "seg_idx": np.int32, "arrived": np.uint8}

    def set_latency(self, ticks=None, max_ticks=None):
        """Per-env observation latency in ticks (``trs_set_latency``): ``ticks`` is a scalar or one value per env, each in ``[0, max_ticks]``
        (``max_ticks`` defaults to the largest value, at least 1; at most 30).  ``None``: off.  ``fetch``, ``fetch_outputs`` and ``device_array`` keep
        showing what the simulator did; ``observation()`` / ``device_observation()`` show what each car is told, ``ticks`` steps late, and
        ``step_pilot`` drives on that.  The history restarts here and at ``load_track``, not at resets.  Launch mode only."""
        if not getattr(self.api, "has_latency", False):
            raise RuntimeError("the oracle has no observation latency (trs_set_latency): it is a view on the truth the oracle checks, HIP library only")
        if ticks is None:
            self.api.check(self.api.set_latency(self._h, None, 0), "set_latency")
            return
        t = np.asarray(ticks)
        if t.dtype.kind not in "iu" and not np.all(t == np.round(t)):
            raise ValueError("latency ticks must be whole numbers")
        t = np.ascontiguousarray(np.broadcast_to(t.astype(np.int64), (self.n,)))
        if np.any(t < -2**31) or np.any(t >= 2**31):
            raise ValueError("latency ticks out of range")
        t = np.ascontiguousarray(t, dtype=np.int32)
        m = max(1, int(t.max())) if max_ticks is None else int(max_ticks)
        self.api.check(self.api.set_latency(self._h, t.ctypes.data, m), "set_latency")

    def latency(self):
        """``(ticks int32[n_envs], max_ticks)`` (``trs_get_latency``); ``max_ticks == 0``: off."""
        if not getattr(self.api, "has_latency", False):
            raise RuntimeError("the oracle has no observation latency (trs_get_latency)")
        t, m = np.zeros(self.n, np.int32), C.c_int(0)
        self.api.check(self.api.get_latency(self._h, t.ctypes.data, C.byref(m)), "get_latency")
        return t, int(m.value)

    def observation(self, image=True):
        """``(img, x, y, z, speed, cte, seg_idx, arrived)`` of all envs as fresh numpy arrays in one synchronisation (``trs_fetch_observation``):
        ``fetch_outputs`` as the cars are told it; zeros and ``arrived == 0`` for an env whose first observation is still under way."""
        n = self.n
        img = np.empty((n, self.H, self.W, 3), np.uint8) if image else None
        f = [np.empty(n, np.float32) for _ in range(5)]
        seg, arrived = np.empty(n, np.int32), np.empty(n, np.uint8)
        self.api.check(self.api.fetch_observation(self._h, img.ctypes.data if image else None, *[a.ctypes.data for a in f],
                                                  seg.ctypes.data, arrived.ctypes.data), "fetch_observation")
        return (img, *f, seg, arrived)

    def observation_view(self):
        ov = _ffi.TrsObsView()
        self.api.check(self.api.get_observation(self._h, C.byref(ov)), "get_observation")
        return ov

    def device_observation(self, name, stream=None, sync=True):
        """Zero-copy handle on one field of the observation (``trs_get_observation``): ``img``, ``depth``, ``pos_x``, ``pos_y``, ``pos_z``,
        ``speed``, ``cte``, ``seg_idx`` or ``arrived``; ordered like ``device_array``.  Read-only, and valid while the NEXT step runs, not beyond.
        With one latency for all envs ``img`` points into the ring slot of the delayed step: no frame byte has been moved."""
        if stream is not None:
            self.api.check(self.api.stream_signal_external(self._h, _stream_ptr(stream) or None), "stream_signal_external")
        elif sync:
            self.sync()
        ptr = getattr(self.observation_view(), name)
        if not ptr:
            raise RuntimeError(f"{name} is not part of this env's observation")
        return _DevicePtr(ptr, self._shape(name), self._OBS_DTYPES[name], self)

    def set_frame_filter(self, cfg=None, enabled=True):
        """``ImgPreprocessing`` fused behind the rasteriser (``trs_set_frame_filter``): from the next frame on, the
        env's ``img`` IS ``cam/processed_img`` at no extra cost (the palette is filtered, not the pixels).  Trim and
        HSV masks only; dynamic brightness and Canny are refused.  ``enabled=False`` returns to raw frames."""
        if not enabled:
            self.api.check(self.api.set_frame_filter(self._h, None), "set_frame_filter")
            return
        pc = cfg if isinstance(cfg, _ffi.TrsPreConfig) else self.pre_config(cfg)
        self.api.check(self.api.set_frame_filter(self._h, C.byref(pc)), "set_frame_filter")

    def normalize_host(self, frames):
        """Pilot-side ``float32(img) / 255`` (``keras_pilot.py:49-55``) -> ``float32[n,H,W,3]``."""
        src = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, self.H, self.W, 3)
        dst = np.empty(src.shape, dtype=np.float32)
        self.api.check(self.api.normalize_host(self._h, src.ctypes.data, dst.ctypes.data, int(src.shape[0])), "normalize_host")
        return dst

    # -- tub images (include/trsim_spec.h, "tub image (JPEG)") ------------------------------------
    def jpeg_header_bytes(self, quality=75):
        if not getattr(self.api, "has_jpeg", False):
            raise RuntimeError("this library has no JPEG encoder (trs_encode_jpeg)")
        n = self.api.jpeg_header_bytes(self._h, int(quality))
        if n < 0:
            self.api.check(n, "jpeg_header_bytes")
        return int(n)

    def jpeg_default_cap(self, quality=75):
        """Bytes per frame ``encode_jpeg`` reserves unless told otherwise: the header, the end marker and a quarter of the raw frame."""
        return self.jpeg_header_bytes(quality) + 2 + self.H * self.W * 3 // 4

    def device_encode_jpeg(self, d_dst, d_len, frames=None, n_images=None, quality=75, cap=None):
        """``trs_encode_jpeg``, device to device and asynchronous on the env's stream: ``d_dst`` takes ``n_images`` slots of ``cap`` bytes, ``d_len``
        int32 lengths (negated where a file did not fit).  ``frames``: ``None`` = the latest frames, else a device ``uint8[n,H,W,3]``; pointers are
        integers or anything with ``__cuda_array_interface__`` (torch tensors)."""
        src = device_ptr(frames)
        n = self.n if n_images is None else int(n_images)
        cap = self.jpeg_default_cap(quality) if cap is None else int(cap)
        if not getattr(self.api, "has_jpeg", False):
            raise RuntimeError("this library has no JPEG encoder (trs_encode_jpeg)")
        self.api.check(self.api.encode_jpeg(self._h, src, n, int(quality), device_ptr(d_dst), cap, device_ptr(d_len)), "encode_jpeg")
        return cap

    def encode_jpeg(self, frames=None, quality=75, cap=None):
        """The ``img_k.jpg`` bytes of N frames in one call (``trs_encode_jpeg_host``) as a ``JpegFrames`` sequence — byte for byte what
        ``Image.fromarray(frame).save(path, quality=quality)`` writes.  ``frames``: ``None`` = the env's latest frames, a device array, or a host
        ``uint8[n,H,W,3]`` (uploaded first).  A frame whose file exceeds ``cap`` bytes (default: header + 2 + H*W*3/4) is encoded with Pillow from
        the fetched frame when Pillow imports; otherwise the call raises and names the frame."""
        if not getattr(self.api, "has_jpeg", False):
            raise RuntimeError("this library has no JPEG encoder (trs_encode_jpeg)")
        host = None
        if frames is None:
            src, n = None, self.n
        elif is_device_array(frames):
            shape = tuple(frames.__cuda_array_interface__["shape"])
            if shape[-3:] != (self.H, self.W, 3):
                raise ValueError(f"frames must be uint8[n, {self.H}, {self.W}, 3]")
            src, n = device_ptr(frames), int(np.prod(shape[:-3], dtype=np.int64))
        else:
            host = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, self.H, self.W, 3)
            n = int(host.shape[0])
            d = C.c_void_p()
            self.api.check(self.api.scratch(self._h, SLOT_JPEG_IN, host.nbytes, C.byref(d)), "scratch")
            self.api.check(self.api.upload(self._h, d, host.ctypes.data, host.nbytes), "upload")
            src = d.value
        cap = self.jpeg_default_cap(quality) if cap is None else int(cap)
        blob = np.empty(max(n, 0) * max(cap, 0), np.uint8)
        off, ln = np.zeros(max(n, 0) + 1, np.int64), np.zeros(max(n, 0), np.int32)
        self.api.check(self.api.encode_jpeg_host(self._h, src, n, int(quality), cap, blob.ctypes.data, blob.nbytes, off.ctypes.data, ln.ctypes.data),
                       "encode_jpeg_host")
        late = {}
        over = np.flatnonzero(ln < 0)
        if over.size:
            try:
                from PIL import Image
            except ImportError:
                raise RuntimeError(f"the JPEG file of env {int(over[0])} takes {-int(ln[over[0]])} bytes, more than cap = {cap}, and Pillow is not "
                                   "there to encode it on the host: pass a larger cap") from None
            import io
            if host is None:
                host = self.fetch("img") if frames is None else None
            for i in over:
                if host is not None:
                    img = host[i]
                else:                                            # a caller's device array: fetch the one frame
                    import torch
                    img = torch.as_tensor(frames, device=f"cuda:{self.device}").reshape(-1, self.H, self.W, 3)[int(i)].cpu().numpy()
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, format="JPEG", quality=int(quality))
                late[int(i)] = buf.getvalue()
        return JpegFrames(blob[:int(off[-1])], off, ln, late)

    # -- tub images, read back (include/trsim_spec.h, "tub image (JPEG), decoding") ----------------
    JPEG_STATUS = {0: "decoded", 1: "skipped", 2: "unsupported", 3: "size differs", 4: "corrupt"}

    def device_decode_jpeg(self, d_files, d_off, d_len, d_dst, d_status, n_images=None):
        """``trs_decode_jpeg``, device to device and asynchronous on the env's stream: file ``i`` is ``d_files[d_off[i] : d_off[i] + d_len[i]]``
        (``d_off`` int64, ``d_len`` int32 — the encoder's slots with ``d_off[i] = i * cap`` and its ``d_len``, or a packed blob), ``d_dst`` takes
        ``uint8[n,H,W,3]``, ``d_status`` int32 per file (``JPEG_STATUS``).  Pointers are integers or anything with ``__cuda_array_interface__``."""
        if not getattr(self.api, "has_jpeg_decode", False):
            raise RuntimeError("this library has no JPEG decoder (trs_decode_jpeg)")
        n = self.n if n_images is None else int(n_images)
        self.api.check(self.api.decode_jpeg(self._h, device_ptr(d_files), device_ptr(d_off), device_ptr(d_len), n, device_ptr(d_dst), device_ptr(d_status)),
                       "decode_jpeg")

    def decode_jpeg(self, files):
        """The frames of N ``img_k.jpg`` files in one call (``trs_decode_jpeg_host``) -> ``(uint8[n,H,W,3], int32 status[n])`` — byte for byte what
        ``np.asarray(Image.open(path))`` gives.  ``files``: a sequence of ``bytes`` or a ``JpegFrames``.  A file the device reports as unsupported
        (status 2: progressive, grayscale, other sampling, ...) is decoded with Pillow on the host when its result has the shape (H, W, 3); otherwise,
        and for a file of another size (3) or a corrupt one (4), the call raises and names the index."""
        if not getattr(self.api, "has_jpeg_decode", False):
            raise RuntimeError("this library has no JPEG decoder (trs_decode_jpeg)")
        files = [bytes(f) for f in files]
        n = len(files)
        out = np.zeros((n, self.H, self.W, 3), np.uint8)
        status = np.zeros(n, np.int32)
        if n == 0:
            return out, status
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(f) for f in files], out=off[1:])
        blob = np.frombuffer(b"".join(files) or b"\0", np.uint8)
        self.api.check(self.api.decode_jpeg_host(self._h, blob.ctypes.data, off.ctypes.data, n, out.ctypes.data, status.ctypes.data), "decode_jpeg_host")
        for i in np.flatnonzero(status != 0):
            i, st = int(i), int(status[i])
            img = None
            if st == 2:
                try:
                    import io
                    from PIL import Image
                    img = np.asarray(Image.open(io.BytesIO(files[i])))
                except Exception:
                    img = None
            if img is None or img.shape != (self.H, self.W, 3) or img.dtype != np.uint8:
                raise RuntimeError(f"the JPEG file of index {i} is {self.JPEG_STATUS.get(st, st)} (status {st}, {len(files[i])} bytes) and cannot be decoded "
                                   f"to uint8[{self.H}, {self.W}, 3]" + (" on the host either" if st == 2 else ""))
            out[i] = img
        return out, status

    # -- camera codec (include/trsim_spec.h, "camera codec (JPEG round trip)") ---------------------
    def _need_codec(self):
        if not getattr(self.api, "has_jpeg_codec", False):
            raise RuntimeError("this library has no camera codec (trs_jpeg_roundtrip)")

    def device_jpeg_roundtrip(self, frames=None, quality=75, d_dst=None, n_images=None):
        """``trs_jpeg_roundtrip``, device to device and asynchronous on the env's stream: ``frames`` (``None`` = the latest frames, else a device
        ``uint8[n,H,W,3]``) as a JPEG save at ``quality`` and open would give them back.  ``d_dst``: ``None`` = the env's own codec buffer (which
        ``step_pilot`` also writes while a camera codec is set), else a device ``uint8[n,H,W,3]`` that does not overlap ``frames``.  Returns a
        zero-copy handle on the result."""
        self._need_codec()
        if frames is not None and n_images is None and is_device_array(frames):
            shape = tuple(frames.__cuda_array_interface__["shape"])
            if shape[-3:] != (self.H, self.W, 3):
                raise ValueError(f"frames must be uint8[n, {self.H}, {self.W}, 3]")
            n_images = int(np.prod(shape[:-3], dtype=np.int64))
        n = self.n if n_images is None else int(n_images)
        out = C.c_void_p()
        self.api.check(self.api.jpeg_roundtrip(self._h, device_ptr(frames), n, int(quality), device_ptr(d_dst), C.byref(out)), "jpeg_roundtrip")
        return _DevicePtr(out.value, (n, self.H, self.W, 3), np.uint8, self if d_dst is None else d_dst)

    def jpeg_roundtrip(self, frames=None, quality=75):
        """``codec(frame, quality)`` of N frames as a fresh ``uint8[n,H,W,3]`` (``trs_jpeg_roundtrip_host``) — byte for byte what saving each frame
        with Pillow at ``quality`` and opening the file gives, the lossy frame the reference's pilot sees.  ``frames``: ``None`` = the env's latest
        frames, a device array, or a host ``uint8[n,H,W,3]``."""
        self._need_codec()
        if frames is not None and is_device_array(frames):
            d = self.device_jpeg_roundtrip(frames, quality)
            import torch
            self.sync()
            return torch.as_tensor(d, device=f"cuda:{self.device}").cpu().numpy()
        src = None if frames is None else np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, self.H, self.W, 3)
        n = self.n if src is None else int(src.shape[0])
        dst = np.empty((n, self.H, self.W, 3), np.uint8)
        self.api.check(self.api.jpeg_roundtrip_host(self._h, None if src is None else src.ctypes.data, n, int(quality), dst.ctypes.data), "jpeg_roundtrip_host")
        return dst

    def set_camera_codec(self, quality=75):
        """While set (``trs_set_camera_codec``), ``step_pilot`` feeds the pilot ``codec(frame, quality)`` of the frame it reads — the latest one, or
        the delayed observation while a latency is set; ``fetch``, ``fetch_outputs``, ``observation`` and ``encode_jpeg`` keep showing the rendered
        truth.  ``0`` or ``None``: off.  Refused while a frame filter is set, and ``set_frame_filter`` is refused while a codec is set."""
        self._need_codec()
        self.api.check(self.api.set_camera_codec(self._h, int(quality or 0)), "set_camera_codec")

    def camera_codec(self):
        """The quality ``set_camera_codec`` set (``trs_get_camera_codec``); 0: none."""
        self._need_codec()
        q = C.c_int(0)
        self.api.check(self.api.get_camera_codec(self._h, C.byref(q)), "get_camera_codec")
        return int(q.value)

    def driver_assist_host(self, steering, throttle, brake, speed, mode="steering", k=5):
        """``DriverAssistance.step`` (``components/driver_assistance.py:13-31``) for N cars on the device; returns new float32 arrays."""
        arrs = [np.array(a, dtype=np.float32, copy=True).reshape(-1) for a in (steering, throttle, brake, speed)]
        n = arrs[0].size
        self.api.check(self.api.driver_assist_host(self._h, {"steering": 0, "speed": 1}[mode], float(k), arrs[0].ctypes.data, arrs[1].ctypes.data,
                                                    arrs[2].ctypes.data, arrs[3].ctypes.data, n), "driver_assist_host")
        return arrs[0], arrs[1], arrs[2]

    # -- ControlMultiplexer for N cars (components/controlmultiplexer.py:24-43) --------------------
    MODES = {"human": 0, "ai_steering": 1, "ai": 2}

    def mux_config(self, cfg=None, loop_hz=20):
        """``trs_mux_config`` from the reference's ``ai_launch_*`` keys (``core/config.py:57-63``); a duration in
        seconds becomes ``ceil(duration * loop_hz)`` ticks of the fixed-step env (at least 1)."""
        import math
        mc = _ffi.TrsMuxConfig()
        self.api.default_mux_config(C.byref(mc))
        cfg = cfg or {}
        mc.throttle_lock_enabled = int(bool(cfg.get("ai_launch_boost_throttle_enabled", False)))
        mc.throttle_lock_value = float(cfg.get("ai_launch_boost_throttle_value", 1.0))
        mc.throttle_lock_ticks = max(1, math.ceil(float(cfg.get("ai_launch_boost_throttle_duration", 5)) * loop_hz))
        mc.steering_lock_enabled = int(bool(cfg.get("ai_launch_lock_steering_enabled", False)))
        mc.steering_lock_value = float(cfg.get("ai_launch_lock_steering_value", 0.0))
        mc.steering_lock_ticks = max(1, math.ceil(float(cfg.get("ai_launch_lock_steering_duration", 3)) * loop_hz))
        return mc

    @classmethod
    def encode_modes(cls, modes):
        """``usr/mode`` values (``DriveMode`` members, their ``.value`` strings or the integers 0..2) -> uint8 codes;
        anything else becomes 255 = 'leave this car's outputs alone'."""
        if isinstance(modes, np.ndarray) and modes.dtype == np.uint8:
            return np.ascontiguousarray(modes).reshape(-1)
        out = np.empty(len(modes), np.uint8)
        for i, m in enumerate(modes):
            m = getattr(m, "value", m)
            if isinstance(m, str):
                out[i] = cls.MODES.get(m, 255)
            elif isinstance(m, (int, np.integer)) and 0 <= int(m) <= 2:
                out[i] = int(m)
            else:
                out[i] = 255
        return out

    def control_mux_host(self, modes, usr, ai, keep=None, cfg=None, loop_hz=20):
        """One tick of ``ControlMultiplexer.step`` for n cars on the device.  ``usr`` / ``ai``: (steering, throttle,
        breaking) arrays; ``keep``: the values a car with an unknown mode retains (default zeros).  Returns the three
        ``mux/*`` arrays (float32)."""
        mode = self.encode_modes(modes)
        n = mode.size
        f = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), (n,)))
        ins = [f(a) for a in (*usr, *ai)]
        outs = [np.array(f(a), copy=True) for a in (keep if keep is not None else (0.0, 0.0, 0.0))]
        mc = cfg if isinstance(cfg, _ffi.TrsMuxConfig) else self.mux_config(cfg, loop_hz)
        self.api.check(self.api.control_mux_host(self._h, C.byref(mc), mode.ctypes.data, *[a.ctypes.data for a in ins],
                                                 *[a.ctypes.data for a in outs], n), "control_mux_host")
        return tuple(outs)

    def control_mux_reset(self):
        self.api.check(self.api.control_mux_reset(self._h), "control_mux_reset")

    # -- pilot in the loop (cnn_2d_speed_control) -------------------------------------------------
    def pilot_load(self, weights):
        """``weights``: 22 float32 arrays — kernel, bias of conv1..conv7, dense1..dense3, output_layer in Keras
        layouts (``[KH][KW][CIN][COUT]`` / ``[IN][OUT]``), e.g. ``model.get_weights()`` of the reference's
        ``Keras_2D_CNN.get_model(input_shape, 2)`` (``components/keras_train.py:127-174``)."""
        if isinstance(weights, dict):
            # by layer name: {"conv1": (kernel, bias), ...}.  For the model types with several inputs this is the safe form: the
            # order of model.get_weights() follows Keras's layer sorting, the library's order is fixed by name (include/trsim.h)
            names = _ffi.PILOT_LAYERS[2 * len(weights)]
            missing = [nm for nm in names if nm not in weights]
            if missing:
                raise ValueError(f"weights lack the layers {missing}")
            weights = [a for nm in names for a in weights[nm]]
        arrs = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        self.api.check(self.api.pilot_load(self._h, ptrs, len(arrs)), "pilot_load")
        self._pilot_arrays = arrs                                    # what pilot_train_begin and pilot_weights start from

    def pilot_tuning(self, **choices):
        """Override kernel choices of the NEXT ``pilot_load`` (``trs_pilot_tuning``, include/trsim.h) — tests that compare a kernel
        with the one it replaced, and measurements.  No arguments: back to the defaults."""
        if not choices:
            self.api.check(self.api.pilot_set_tuning(self._h, None), "pilot_set_tuning")
            return
        t = _ffi.TrsPilotTuning()
        self.api.default_pilot_tuning(C.byref(t))
        names = {f[0] for f in _ffi.TrsPilotTuning._fields_} - {"struct_size"}
        for k, v in choices.items():
            if k not in names:
                raise ValueError(f"trs_pilot_tuning has no field {k!r}")
            setattr(t, k, int(v))
        self.api.check(self.api.pilot_set_tuning(self._h, C.byref(t)), "pilot_set_tuning")

    def resident_lifetime(self, life_us):
        """Test hook (``trs_resident_debug_lifetime``): resident workers leave by themselves after ``life_us``.  Only in the test build of the library
        (``csrc/libtrsim_testhooks.so``, ``-DTRS_TEST_HOOKS``): bind it with ``BatchedEnv(_api=...)`` as ``tests/conftest.py`` does."""
        if not getattr(self.api, "has_test_hooks", False):
            raise RuntimeError("trs_resident_debug_lifetime is not part of libtrsim.so: bind csrc/libtrsim_testhooks.so (tests/conftest.py: make_env('hip_hooks', ...))")
        self.api.check(self.api.resident_debug_lifetime(self._h, int(life_us)), "resident_debug_lifetime")

    def resident_abort(self):
        """Test hook (``trs_resident_debug_abort``): the running worker's abort bit is set from outside (test build of the library only)."""
        if not getattr(self.api, "has_test_hooks", False):
            raise RuntimeError("trs_resident_debug_abort is not part of libtrsim.so: bind csrc/libtrsim_testhooks.so (tests/conftest.py: make_env('hip_hooks', ...))")
        self.api.check(self.api.resident_debug_abort(self._h), "resident_debug_abort")

    def pilot_config(self, cfg=None):
        pc = _ffi.TrsPilotConfig()
        self.api.default_pilot_config(C.byref(pc))
        cfg = cfg or {}
        pc.spd_ctl_threshold = float(cfg.get("spd_ctl_threshold", 1.1))
        pc.spd_ctl_break = int(bool(cfg.get("spd_ctl_break", False)))
        pc.spd_ctl_reverse_multiplier = float(cfg.get("spd_ctl_reverse_multiplier", 1.0))
        pc.spd_ctl_break_multiplier = float(cfg.get("spd_ctl_break_multiplier", 1.0))
        pc.smooth_steering_enabled = int(bool(cfg.get("smooth_steering_enabled", False)))
        pc.smooth_steering_threshold = float(cfg.get("smooth_steering_threshold", 0.9))
        mt = getattr(cfg.get("model_type", "cnn_2d_speed_control"), "value", cfg.get("model_type", "cnn_2d_speed_control"))
        if mt not in _ffi.PILOT_MODEL_TYPES:
            raise ValueError(f"model_type {mt!r}: the GPU pilot runs {sorted(_ffi.PILOT_MODEL_TYPES)}")
        pc.model_type = _ffi.PILOT_MODEL_TYPES[mt]
        return pc

    def pilot_forward_host(self, frames, speed=None, segment=None):
        """Raw model outputs ``float32[n, 2]`` for host frames ``uint8[n,H,W,3]``; ``speed`` ('gym/speed', divided by 20 inside)
        for ``cnn_2d_speed_as_feature``, ``speed`` and ``segment`` ('loc/segment') for ``cnn_2d_full_house``."""
        src = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, self.H, self.W, 3)
        n = int(src.shape[0])
        out = np.empty((n, 2), dtype=np.float32)
        if speed is None and segment is None:
            self.api.check(self.api.pilot_forward_host(self._h, src.ctypes.data, n, out.ctypes.data), "pilot_forward_host")
            return out
        f = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), (n,)))
        sp, sg = f(speed), f(segment)
        self.api.check(self.api.pilot_forward_host_ex(self._h, src.ctypes.data, None if sp is None else sp.ctypes.data,
                                                      None if sg is None else sg.ctypes.data, n, out.ctypes.data), "pilot_forward_host_ex")
        return out

    def pilot_layer(self, layer, shape):
        out = np.empty(shape, dtype=np.float32)
        self.api.check(self.api.pilot_debug_layer(self._h, int(layer), out.ctypes.data, out.size), "pilot_debug_layer")
        return out

    def pilot_range_check(self):
        """fp16 saturations of the last forward pass per convolution (``trs_pilot_range_check``): ``uint64[8]``, [0..6] = conv1..conv7, [7] = sum."""
        out = np.zeros(8, np.uint64)
        self.api.check(self.api.pilot_range_check(self._h, out.ctypes.data), "pilot_range_check")
        return out

    def step_pilot(self, n_steps=1, cfg=None):
        """Closed loop: controls = KerasPilot.step(previous frame, speed), then one env step; all on the device.  With ``set_latency`` the pilot
        sees each car's observation (frame, speed, segment) instead, and cars nothing has reached yet get (0, 0, 0).  With ``set_camera_codec`` the
        frame it sees has been through the JPEG round trip first."""
        pc = cfg if isinstance(cfg, _ffi.TrsPilotConfig) else self.pilot_config(cfg)
        self.api.check(self.api.step_pilot(self._h, C.byref(pc), int(n_steps)), "step_pilot")

    # -- training the pilot's tail (include/trsim_spec.h, "training the pilot's tail") -----------------------------------------
    def _need_train(self):
        if not getattr(self.api, "has_train", False):
            raise RuntimeError("this library cannot train the pilot's tail (trs_pilot_train_step): HIP library only")
        if getattr(self, "_pilot_arrays", None) is None:
            raise RuntimeError("no pilot loaded: pilot_load first")

    def _train_side(self):
        """True when the loaded pilot is the 28-array type (``cnn_2d_speed_as_feature``): 14 trained arrays, a feature per frame."""
        return len(self._pilot_arrays) == 28

    def _train_arrays(self):
        """The trained arrays' places in ``pilot_load``'s list: 14 .. 21 for a 22-array pilot, 14 .. 27 for a 28-array one."""
        return slice(14, 28 if self._train_side() else 22)

    def train_config(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, layers=None):
        """``trs_train_config``: Adam's constants (Keras's ``optimizers.Adam(lr=0.001)`` by default) and the layers that move — ``layers``: names
        out of ``_ffi.TRAIN_LAYERS`` (``None``: all four); with a 28-array pilot loaded, out of ``_ffi.TRAIN_SIDE_LAYERS``, which adds
        ``"feature1"`` .. ``"feature3"`` (``None``: all seven)."""
        c = _ffi.TrsTrainConfig()
        self.api.default_train_config(C.byref(c))
        c.lr, c.beta1, c.beta2, c.eps = float(lr), float(beta1), float(beta2), float(eps)
        names = _ffi.TRAIN_SIDE_LAYERS if getattr(self, "_pilot_arrays", None) is not None and self._train_side() else _ffi.TRAIN_LAYERS
        if layers is not None:
            unknown = [nm for nm in layers if nm not in names]
            if unknown:
                raise ValueError(f"layers must come from {names}: {unknown}")
            c.train_mask = sum(1 << names.index(nm) for nm in set(layers))
        else:
            c.train_mask = (1 << len(names)) - 1
        return c

    def dropout_config(self, rate=0.1, sites=None, seed=0):
        """``trs_dropout_config``: the rate, the sites — names out of ``_ffi.DROPOUT_SITES`` (``"x7"``: conv7's output, ``"a1"`` .. ``"a3"``:
        relu(z1) .. relu(z3)) or the bit mask itself; ``None``: all four — and the seed of the draws."""
        if not getattr(self.api, "has_dropout", False):
            raise RuntimeError("this library has no dropout (trs_pilot_train_dropout): HIP library only")
        c = _ffi.TrsDropoutConfig()
        self.api.default_dropout_config(C.byref(c))
        c.rate, c.seed = float(rate), int(seed)
        if sites is not None:
            if isinstance(sites, int):
                c.sites = sites
            else:
                unknown = [nm for nm in sites if nm not in _ffi.DROPOUT_SITES]
                if unknown:
                    raise ValueError(f"dropout_sites must come from {_ffi.DROPOUT_SITES}: {unknown}")
                c.sites = sum(1 << _ffi.DROPOUT_SITES.index(nm) for nm in set(sites))
        return c

    def pilot_train_dropout_keep(self, t, site, n, rate=None, seed=None):
        """The keep flags of step ``t`` (the session's first step is 1) at ``site`` (0..3 or a name out of ``_ffi.DROPOUT_SITES``) for the first ``n``
        frame slots of a batch: ``bool[n, width]``, width F, 100, 50, 25 (``trs_train_dropout_keep``: host arithmetic, no GPU work).  ``rate`` and
        ``seed``: ``None`` takes what the last ``pilot_train_begin(dropout=...)`` of this handle was given."""
        self._need_train()
        site = _ffi.DROPOUT_SITES.index(site) if isinstance(site, str) else int(site)
        last = getattr(self, "_train_dropout", None)
        if (rate is None or seed is None) and last is None:
            raise RuntimeError("no session with dropout on this handle: pass rate and seed")
        cfg = self.dropout_config(last[0] if rate is None else rate, None, last[1] if seed is None else seed)
        flatten = int(self._pilot_arrays[14].shape[0]) - (16 if self._train_side() else 0)    # site 0 masks x7 alone: the branch joins behind that Dropout
        width = flatten if site == 0 else (100, 50, 25)[site - 1] if 1 <= site <= 3 else 0
        keep = np.empty((max(int(n), 0), width), np.uint8)
        self.api.check(self.api.train_dropout_keep(C.byref(cfg), int(t), site, int(n), width, keep.ctypes.data), "train_dropout_keep")
        return keep.astype(bool)

    def pilot_train_begin(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, layers=None, convs=None, dropout=None, dropout_sites=None, dropout_seed=0):
        """Open a training session on the loaded pilot's dense tail (``trs_pilot_train_begin``): fp32 master weights from the arrays ``pilot_load``
        was given, Adam's moments at zero.  With a 28-array pilot (``cnn_2d_speed_as_feature``) the session also trains feature1 .. feature3 and
        dense1's rows behind the flatten (``trs_pilot_train_begin_ex``), and every step takes the feature; ``cnn_2d_full_house`` is refused.  ``convs``: names out of ``_ffi.TRAIN_CONV_LAYERS`` (``"conv4"`` ..
        ``"conv7"``) that are trained as well (``trs_pilot_train_convs``); ``None``: the convolutions stay as loaded.  conv1 .. conv3 always do.
        ``dropout``: the rate of training-mode dropout behind conv7 and the three hidden dense layers (``trs_pilot_train_dropout``; the reference's
        is 0.1), ``dropout_sites`` the sites (``dropout_config``; ``None``: all four), ``dropout_seed`` the seed of the draws; ``None``: no
        dropout.  Inference never drops.
        Until ``pilot_train_end`` the handle refuses ``pilot_load`` and ``pilot_tuning``; it drives with the current weights all along."""
        self._need_train()
        cfg = self.train_config(lr, beta1, beta2, eps, layers)
        drop = None if dropout is None else self.dropout_config(dropout, dropout_sites, dropout_seed)
        mask = 0
        if convs is not None:
            unknown = [nm for nm in convs if nm not in _ffi.TRAIN_CONV_LAYERS]
            if unknown:
                raise ValueError(f"convs must come from {_ffi.TRAIN_CONV_LAYERS}: {unknown}")
            mask = sum(1 << _ffi.TRAIN_CONV_LAYERS.index(nm) for nm in set(convs))
        tail = self._pilot_arrays[self._train_arrays()]
        ptrs = (C.c_void_p * len(tail))(*[a.ctypes.data for a in tail])
        if len(self._pilot_arrays) == 22:
            self.api.check(self.api.pilot_train_begin(self._h, C.byref(cfg), ptrs), "pilot_train_begin")
        else:                                                           # (a 42-array pilot: the library's refusal)
            self.api.check(self.api.pilot_train_begin_ex(self._h, C.byref(cfg), ptrs, len(tail)), "pilot_train_begin_ex")
        self._train_convs = False
        self._train_dropout = None

        def second(rc, what):
            if rc != 0:
                why = self.api.last_error()                             # the refusal's own text, before another call of the library replaces it
                self.api.pilot_train_end(self._h)                       # no half-open session behind a refusal
                raise RuntimeError(f"{self.api.prefix}{what} failed ({rc}): {why.decode() if why else ''}")

        if convs is not None:                                           # (an empty list: the library's refusal of a zero mask)
            cptrs = (C.c_void_p * 8)(*[a.ctypes.data for a in self._pilot_arrays[6:14]])
            second(self.api.pilot_train_convs(self._h, mask, cptrs), "pilot_train_convs")
            self._train_convs = True
        if drop is not None:
            second(self.api.pilot_train_dropout(self._h, C.byref(drop)), "pilot_train_dropout")
            self._train_dropout = (float(dropout), int(dropout_seed))

    def pilot_train_step(self, frames, labels, n=None, loss=None, features=None):
        """One Adam step on ``frames uint8[n, H, W, 3]`` and ``labels float32[n, 2]`` on the device (torch tensors, anything with
        ``__cuda_array_interface__``, or device pointers with ``n``), ``n <= n_envs``.  Asynchronous on the env's stream.  ``loss``: a device
        float32 the batch's loss (before the update) is written to, and the call returns ``None``; without it the call waits and returns the loss.
        ``features``: ``float32[n, 1]`` on the device, speed / 20 per frame as the ``speed_feature`` loader delivers it: required by the session of a
        28-array pilot (``trs_pilot_train_step_ex``), not read by a 22-array one."""
        self._need_train()
        if n is None:
            n = int(frames.shape[0])
        if features is None and not self._train_side():
            self.api.check(self.api.pilot_train_step(self._h, device_ptr(frames), device_ptr(labels), int(n), device_ptr(loss)), "pilot_train_step")
        else:
            self.api.check(self.api.pilot_train_step_ex(self._h, device_ptr(frames), device_ptr(features), device_ptr(labels), int(n), device_ptr(loss)),
                           "pilot_train_step_ex")
        self._train_last_n = int(n)
        if loss is not None:
            return None
        return float(self.pilot_train_debug("loss")[0])

    def pilot_train_debug(self, item, array=0):
        """Item ``item`` (a key of ``_ffi.TRAIN_DEBUG``; ``"m"`` and ``"v"`` take the number of the array, 0..7) of the last training step as a flat
        float32 array (``trs_pilot_train_debug``); the caller reshapes."""
        self._need_train()
        which = _ffi.TRAIN_DEBUG[item] + (int(array) if item in ("m", "v") else 0)
        F = int(self._pilot_arrays[14].shape[0]) - (16 if self._train_side() else 0)     # the flatten's length: the items of dense1's kernel cover its rows
        n = int(getattr(self, "_train_last_n", 0))
        sizes = {"out": 2 * n, "z1": 100 * n, "z2": 50 * n, "z3": 25 * n, "delta1": 100 * n, "delta2": 50 * n, "delta3": 25 * n, "delta4": 2 * n,
                 "gw1": F * 100, "gw2": 5000, "gw3": 1250, "gw4": 50, "gb1": 100, "gb2": 50, "gb3": 25, "gb4": 2, "scale_exp": 1, "loss": 1, "pack1": F * 100,
                 "a1": 100 * n, "a2": 50 * n, "a3": 25 * n}
        size = sizes["gw1"] if item in ("m", "v") and int(array) == 0 else self._pilot_arrays[14 + int(array)].size if item in ("m", "v") else sizes[item]
        out = np.empty(size, np.float32)
        self.api.check(self.api.pilot_train_debug(self._h, which, out.ctypes.data, out.size), "pilot_train_debug")
        return out

    def pilot_train_debug_side(self, item, array=None):
        """Item ``item`` (a key of ``_ffi.TRAIN_SIDE_DEBUG``) of the last training step of a 28-array session as a flat float32 array
        (``trs_pilot_train_debug_side``); ``"g"``, ``"m"`` and ``"v"`` take the side array's name, a key of ``_ffi.TRAIN_SIDE_ARRAYS`` (``"w1y"``: rows
        F .. F + 15 of dense1's kernel)."""
        self._need_train()
        which, per_frame = _ffi.TRAIN_SIDE_DEBUG[item]
        if per_frame is None:
            j, size = _ffi.TRAIN_SIDE_ARRAYS[array]
            which += j
        else:
            size = per_frame * int(getattr(self, "_train_last_n", 0))
        out = np.empty(size, np.float32)
        self.api.check(self.api.pilot_train_debug_side(self._h, which, out.ctypes.data, out.size), "pilot_train_debug_side")
        return out

    def pilot_train_weights(self):
        """``(arrays, t)``: the fp32 master arrays in Keras layouts — the eight of dense1 .. output_layer, and behind them the six of feature1 ..
        feature3 for a 28-array pilot — and the number of steps taken (``trs_pilot_train_get``, ``trs_pilot_train_get_ex``)."""
        self._need_train()
        outs = [np.empty_like(a) for a in self._pilot_arrays[self._train_arrays()]]
        ptrs = (C.c_void_p * len(outs))(*[a.ctypes.data for a in outs])
        t = C.c_int(0)
        if len(outs) == 8:
            self.api.check(self.api.pilot_train_get(self._h, ptrs, C.byref(t)), "pilot_train_get")
        else:
            self.api.check(self.api.pilot_train_get_ex(self._h, ptrs, len(outs), C.byref(t)), "pilot_train_get_ex")
        return outs, int(t.value)

    def pilot_train_conv_weights(self):
        """The eight fp32 master arrays of conv4 .. conv7 (kernel ``[3, 3, CIN, COUT]`` and bias each) of a session opened with ``convs``
        (``trs_pilot_train_get_convs``); a layer that is not trained comes back as it was loaded."""
        self._need_train()
        outs = [a.copy() for a in self._pilot_arrays[6:14]]
        ptrs = (C.c_void_p * 8)(*[a.ctypes.data for a in outs])
        self.api.check(self.api.pilot_train_get_convs(self._h, ptrs), "pilot_train_get_convs")
        return outs

    def pilot_train_debug_conv(self, layer, item):
        """Item ``item`` (a key of ``_ffi.TRAIN_CONV_DEBUG``) of ``layer`` (``"conv4"`` .. ``"conv7"``) after the last training step as a flat
        float32 array (``trs_pilot_train_debug_conv``); the caller reshapes."""
        self._need_train()
        j = _ffi.TRAIN_CONV_LAYERS.index(layer)
        kern, n = self._pilot_arrays[6 + 2 * j], int(getattr(self, "_train_last_n", 0))
        ih, iw = self.conv_input_size(j)
        sizes = {"delta": n * (ih - 2) * (iw - 2) * kern.shape[3], "gw": kern.size, "mw": kern.size, "vw": kern.size, "pack": kern.size,
                 "gb": kern.shape[3], "mb": kern.shape[3], "vb": kern.shape[3], "scale_exp": 1}
        out = np.empty(sizes[item], np.float32)
        self.api.check(self.api.pilot_train_debug_conv(self._h, j, _ffi.TRAIN_CONV_DEBUG[item], out.ctypes.data, out.size), "pilot_train_debug_conv")
        return out

    def conv_input_size(self, j):
        """``(IH, IW)`` of conv(4 + j)'s input for this handle's frames: three 5 x 5 stride-2 valid layers, then j 3 x 3 stride-1 ones."""
        h, w = int(self.H), int(self.W)
        for _ in range(3):
            h, w = (h - 5) // 2 + 1, (w - 5) // 2 + 1
        return h - 2 * j, w - 2 * j

    def pilot_train_end(self):
        """Close the session (``trs_pilot_train_end``).  The arrays ``pilot_weights`` returns keep the trained tail and convolutions."""
        self._need_train()
        tail, _ = self.pilot_train_weights()
        convs = self.pilot_train_conv_weights() if getattr(self, "_train_convs", False) else list(self._pilot_arrays[6:14])
        self.api.check(self.api.pilot_train_end(self._h), "pilot_train_end")
        self._train_convs = False
        self._pilot_arrays = list(self._pilot_arrays[:6]) + convs + tail + list(self._pilot_arrays[14 + len(tail):])

    def pilot_weights(self):
        """The arrays given to ``pilot_load`` with the trained ones replaced (the masters of an open session, or what the last session left): ready
        for ``np.savez`` and for ``pilot_load`` of another handle."""
        if getattr(self, "_pilot_arrays", None) is None:
            raise RuntimeError("no pilot loaded: pilot_load first")
        arrs = [a.copy() for a in self._pilot_arrays]
        if getattr(self.api, "has_train", False) and len(arrs) in (22, 28):
            where = self._train_arrays()
            outs = [np.empty_like(a) for a in arrs[where]]
            ptrs = (C.c_void_p * len(outs))(*[a.ctypes.data for a in outs])
            rc = self.api.pilot_train_get(self._h, ptrs, None) if len(outs) == 8 else self.api.pilot_train_get_ex(self._h, ptrs, len(outs), None)
            if rc == 0:                                                 # an open session: its masters (refused without one: the arrays as kept)
                arrs[where] = outs
                if getattr(self, "_train_convs", False):
                    arrs[6:14] = self.pilot_train_conv_weights()
        return arrs

    # -- scripted expert (include/trsim_spec.h, "scripted expert") ----------------------------------------------------------
    def _need_expert(self):
        if not getattr(self.api, "has_expert", False):
            raise RuntimeError("the oracle has no scripted expert (trs_set_expert): its checker is the restatement in tests/test_expert_cpu.py, HIP library only")

    def expert_config(self, **fields):
        """``trs_expert_config`` with the library's defaults (``trs_default_expert_config``) and ``fields`` over them."""
        self._need_expert()
        ec = _ffi.TrsExpertConfig()
        self.api.default_expert_config(C.byref(ec))
        names = {f[0] for f in _ffi.TrsExpertConfig._fields_} - {"struct_size"}
        for k, v in fields.items():
            if k not in names:
                raise ValueError(f"trs_expert_config has no field {k!r}")
            setattr(ec, k, int(v) if k in ("look", "seed") else float(v))
        return ec

    def set_expert(self, cfg=None, target_speed=None, profile=None, **fields):
        """The scripted expert, the stand-in for the reference's human driver (``trs_set_expert``): steer against the cross-track error and the heading
        error ``look`` points ahead, hold a speed.  ``cfg``: ``None`` = the defaults, a ``TrsExpertConfig`` or a dict of its fields; ``fields`` override
        it (``look``, ``k_cte``, ``k_head``, ``thr_hi``, ``thr_lo``, ``brake_over``, ``brake_val``, ``alpha``, ``sigma``, ``seed``).  ``target_speed``: a
        number, or one value per env.  ``profile``: a speed limit per track point, float ``[n_points]`` (e.g. ``corner_speed_profile``).
        ``set_expert(False)`` switches the expert off.  The driver's tick counter and disturbance start from zero; ``load_track`` switches it off."""
        self._need_expert()
        if cfg is False:
            self.api.check(self.api.set_expert(self._h, None, None, None), "set_expert")
            return
        if isinstance(cfg, _ffi.TrsExpertConfig):
            base = {f[0]: getattr(cfg, f[0]) for f in _ffi.TrsExpertConfig._fields_ if f[0] != "struct_size"}
        else:
            base = dict(cfg or {})
        base.update(fields)
        tg = None
        if target_speed is not None:
            t = np.asarray(target_speed, dtype=np.float32)
            if t.ndim == 0:
                base["target_speed"] = float(t)
            else:
                if t.shape != (self.n,):
                    raise ValueError(f"target_speed must be a number or have shape ({self.n},)")
                tg = np.ascontiguousarray(t)
        pf = None
        if profile is not None:
            pf = np.ascontiguousarray(profile, dtype=np.float32)
            if pf.shape != (self.n_points,):
                raise ValueError(f"profile must have one value per track point: shape ({self.n_points},)")
        ec = self.expert_config(**base)
        self.api.check(self.api.set_expert(self._h, C.byref(ec), None if tg is None else tg.ctypes.data, None if pf is None else pf.ctypes.data), "set_expert")

    def expert_act(self, n=None):
        """The expert's answer to the state the env is in (``trs_expert_act``): the pure rule, no disturbance, nothing of the driver advances — after
        ``step_pilot`` these are DAgger labels.  Returns three device handles (scratch slots): 'usr/steering', 'usr/throttle', 'usr/breaking'."""
        self._need_expert()
        n = self.n if n is None else int(n)
        outs = [self.scratch(sl, (n,)) for sl in SLOT_EXPERT]
        self.api.check(self.api.expert_act(self._h, *[device_ptr(o) for o in outs], n), "expert_act")
        return tuple(outs)

    def step_expert(self, n_steps=1, capture=None):
        """Closed loop on the device (``trs_step_expert``): per tick the expert's controls — the label plus its slowly varying steering disturbance
        (``sigma``) — go into the env's own control arrays (``fetch('ctl_steer')`` ...), then one env step.  ``capture``: a ``TrsExpertCapture`` or a
        dict ``{every, skip, capacity, rows, frames}`` with ``rows`` a device float32 ``[capacity, n_envs, 8]`` and ``frames`` ``None`` or a device
        uint8 ``[capacity, n_envs, H, W, 3]``: tick ``k`` of the driver is captured when ``k >= skip`` and ``(k - skip) % every == 0``.  Returns the
        number of slots this call filled."""
        self._need_expert()
        cap = self._capture(capture)
        got = C.c_int(0)
        self.api.check(self.api.step_expert(self._h, int(n_steps), None if cap is None else C.byref(cap), C.byref(got)), "step_expert")
        return int(got.value)

    @staticmethod
    def _capture(capture):
        """A ``TrsExpertCapture`` from a dict ``{every, skip, capacity, rows, frames}`` (anything else is passed through)."""
        if not isinstance(capture, dict):
            return capture
        cap = _ffi.TrsExpertCapture()
        cap.struct_size = C.sizeof(_ffi.TrsExpertCapture)
        cap.every, cap.skip, cap.capacity = int(capture.get("every", 1)), int(capture.get("skip", 0)), int(capture["capacity"])
        cap.d_frames, cap.d_rows = device_ptr(capture.get("frames")), device_ptr(capture.get("rows"))
        return cap

    # -- pilot in the loop with the expert's labels (include/trsim_spec.h) --------------------------------------------------
    def _need_dagger(self):
        if not getattr(self.api, "has_dagger", False):
            raise RuntimeError("the oracle has no trs_step_dagger: its checker is the restatement in tests/test_dagger_cpu.py, HIP library only")

    def dagger_config(self, beta=0.5, hold=1, expert_speed=True, seed=0):
        """``trs_dagger_config`` from the library's defaults (``trs_default_dagger_config``) with the four fields set."""
        self._need_dagger()
        dc = _ffi.TrsDaggerConfig()
        self.api.default_dagger_config(C.byref(dc))
        dc.beta, dc.hold, dc.expert_speed, dc.seed = float(beta), int(hold), int(expert_speed), int(seed)
        return dc

    def step_dagger(self, n_steps=1, cfg=None, beta=0.5, hold=1, expert_speed=True, seed=0, capture=None):
        """Closed loop on the device with the pilot in it and the expert's labels (``trs_step_dagger``; DAgger).  Per tick the loaded pilot acts exactly
        as in ``step_pilot`` (``cfg`` is the pilot config, as there), the expert of ``set_expert`` labels the truth, and a keyed gate decides per car
        who holds the wheel: the expert with probability ``beta``, constant over blocks of ``hold`` ticks, keyed by ``seed`` and the global env id.
        ``expert_speed=True``: throttle and brake are always the expert's; ``False``: they follow the gate (the speed label of the ``speed_ctl`` and
        ``full_house`` loaders is then the pilot's own speed, not a correction).  ``capture`` as for ``step_expert``: a row is the expert's label, the
        APPLIED steering, speed, cte, segment, done; the frame is the one the pilot was fed (codec's, delayed, or latest).  Returns the slots filled."""
        self._need_dagger()
        pc = cfg if isinstance(cfg, _ffi.TrsPilotConfig) else self.pilot_config(cfg)
        dc = self.dagger_config(beta, hold, expert_speed, seed)
        cap = self._capture(capture)
        got = C.c_int(0)
        self.api.check(self.api.step_dagger(self._h, C.byref(pc), C.byref(dc), int(n_steps), None if cap is None else C.byref(cap), C.byref(got)), "step_dagger")
        return int(got.value)

    def dagger_stats(self, reset=False, to_host=True):
        """How the pilot did under ``step_dagger`` since ``set_expert`` or the last ``reset=True`` (``trs_dagger_stats``): a dict of six float32
        ``[n_envs]`` arrays named by ``_ffi.DAGGER_STATS`` — ticks, ticks the expert drove, sum and max of |cte|, sum of |pilot steering - label|,
        ticks with done set.  ``to_host=False``: the device handle float32 ``[n_envs, 6]`` instead (env-owned, live)."""
        self._need_dagger()
        if not to_host:
            ptr = C.c_void_p()
            self.api.check(self.api.dagger_stats(self._h, None, C.byref(ptr), int(bool(reset))), "dagger_stats")
            return _DevicePtr(ptr.value, (self.n, len(_ffi.DAGGER_STATS)), np.float32, self)
        out = np.empty((self.n, len(_ffi.DAGGER_STATS)), np.float32)
        self.api.check(self.api.dagger_stats(self._h, out.ctypes.data, None, int(bool(reset))), "dagger_stats")
        return {name: np.ascontiguousarray(out[:, i]) for i, name in enumerate(_ffi.DAGGER_STATS)}

    def collect(self, ticks, every=5, skip=20, to_host=False, driver="expert", **dagger):
        """A training set without a byte crossing to the host: ``ticks`` ticks of ``step_expert`` in ONE call, every ``every``-th tick
        from the driver's tick ``skip`` on captured.  Returns ``(frames uint8[N, H, W, 3], rows float32[N, 8])`` (physics-only envs: ``frames`` is
        ``None``), N = captured ticks x n_envs in tick order; a row is ``_ffi.EXPERT_ROW``: the expert's label (steering, throttle, breaking), the
        applied steering, speed, cte, 'loc/segment' and done of the state the frame shows.  Device handles on env-owned memory, valid until the next
        ``collect`` (``to_host=True``: fresh numpy arrays instead).  Feed them to ``recorder.records_for``; put the frames through
        ``device_jpeg_roundtrip`` first for what the reference's pilot would have seen.
        ``driver="pilot"``: the ticks are ``step_dagger``'s instead — the loaded pilot (or its keyed mixture with the expert) drives, the rows hold the
        expert's corrections and the frames are the ones the pilot was fed; ``dagger`` takes ``step_dagger``'s ``cfg``, ``beta``, ``hold``,
        ``expert_speed`` and ``seed``.  ``DeviceDataset.append`` aggregates such a round into an existing set."""
        self._need_expert()
        if driver not in ("expert", "pilot"):
            raise ValueError("driver must be 'expert' or 'pilot'")
        if dagger and driver != "pilot":
            raise ValueError(f"{sorted(dagger)} belong to driver='pilot' (step_dagger)")
        ticks, every, skip = int(ticks), int(every), int(skip)
        if ticks < 1 or every < 1 or skip < 0:
            raise ValueError("ticks >= 1, every >= 1 and skip >= 0 are required")
        capacity = (ticks + every - 1) // every                   # no window of `ticks` ticks holds more due ticks
        render = bool(self.cfg.render)
        rows = self.scratch(SLOT_COLLECT[1], (capacity, self.n, 8), np.float32)
        frames = self.scratch(SLOT_COLLECT[0], (capacity, self.n, self.H, self.W, 3), np.uint8) if render else None
        capture = {"every": every, "skip": skip, "capacity": capacity, "rows": rows, "frames": frames}
        got = self.step_expert(ticks, capture) if driver == "expert" else self.step_dagger(ticks, capture=capture, **dagger)
        rows = _DevicePtr(device_ptr(rows), (got * self.n, 8), np.float32, self)
        if render:
            frames = _DevicePtr(device_ptr(frames), (got * self.n, self.H, self.W, 3), np.uint8, self)
        if not to_host:
            return frames, rows
        return (self.to_host(frames) if render else None), self.to_host(rows)

    def to_host(self, handle):
        """A fresh numpy copy of a device handle of this env (behind everything queued on the env's stream so far)."""
        cai = handle.__cuda_array_interface__
        if int(np.prod(cai["shape"], dtype=np.int64)) == 0:
            return np.zeros(cai["shape"], np.dtype(cai["typestr"]))
        import torch
        self.sync()
        return torch.as_tensor(handle, device=f"cuda:{self.device}").cpu().numpy()

    def dataset(self, frames, rows, loader="speed_ctl", label="expert", split=0.8, seed=0, capacity=None, jpeg_quality=None):
        """A ``DeviceDataset`` (``dataset.py``) holding a COPY of a collection — the handles ``collect`` returns are only valid until the next
        ``collect`` — in torch device storage of ``capacity`` records (``None``: what the collection needs; it grows on ``append``).  ``loader`` and
        ``label`` choose the features and labels as ``recorder.records_for`` does, ``split`` the training share (``n_train = floor(split * n)``),
        ``seed`` the split and every epoch's order.  ``jpeg_quality``: the stored frames go through ``device_jpeg_roundtrip`` once, so the set is what
        a tub would have held.  ``dataset.batches(...)`` then serves shuffled minibatches from it (``trs_sample_batch``), ``dataset.pilot_loss()``
        the validation loss of the loaded HIP pilot; ``frames=None`` makes a physics-only set."""
        from .dataset import DeviceDataset
        ds = DeviceDataset(self, loader=loader, label=label, split=split, seed=seed, capacity=int(capacity or 0), with_frames=frames is not None)
        return ds.append(frames, rows, jpeg_quality=jpeg_quality)

    # -- device-resident part graphs (pilot -> mux -> sim without host copies of frames; car_templates/manage.py:46-75) ------
    def scratch(self, slot, shape, dtype=np.float32):
        """A handle-owned device buffer (``trs_scratch``) as a zero-copy handle; the same slot returns the same memory."""
        shape = tuple(np.atleast_1d(shape).tolist()) if not isinstance(shape, tuple) else shape
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self.api.check(self.api.scratch(self._h, int(slot), nbytes, C.byref(ptr)), "scratch")
        return _DevicePtr(ptr.value, shape, dtype, self)

    def upload(self, dst, values):
        """Host values into a device buffer on the env's stream (``trs_upload``); ``values`` is broadcast to the buffer's shape."""
        cai = dst.__cuda_array_interface__
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.dtype(cai["typestr"])), cai["shape"]))
        self.api.check(self.api.upload(self._h, device_ptr(dst), arr.ctypes.data, arr.nbytes), "upload")

    def counters(self):
        """``(device->host bytes, host->device bytes, steps)`` the library itself has copied / taken since creation."""
        out = (C.c_uint64 * 4)()
        self.api.check(self.api.counters(self._h, C.byref(out)), "counters")
        return int(out[0]), int(out[1]), int(out[2])

    def pilot_act_device(self, frames=None, speed=None, mode=None, cfg=None, n=None, segment=None):
        """``KerasPilot.step`` for n cars on the device (``trs_pilot_act``): frames / speed / mode are device handles (``None`` =
        the env's latest frames / own speed / all cars in an AI mode); returns the three ``ai/*`` handles (scratch slots)."""
        n = self.n if n is None else int(n)
        pc = cfg if isinstance(cfg, _ffi.TrsPilotConfig) else self.pilot_config(cfg)
        outs = [self.scratch(sl, (n,)) for sl in SLOT_AI]
        self.api.check(self.api.pilot_act(self._h, C.byref(pc), device_ptr(frames), device_ptr(speed), device_ptr(segment), device_ptr(mode),
                                          *[device_ptr(o) for o in outs], n), "pilot_act")
        return tuple(outs)

    def control_mux_device(self, mode, usr, ai, cfg=None, loop_hz=20, n=None):
        """One tick of ``ControlMultiplexer.step`` on device arrays (``trs_control_mux``).  ``mode``: uint8 device handle;
        ``usr`` / ``ai``: three device handles each; returns the three ``mux/*`` handles (scratch slots, values of cars with an
        unknown mode are kept from the previous tick)."""
        n = self.n if n is None else int(n)
        mc = cfg if isinstance(cfg, _ffi.TrsMuxConfig) else self.mux_config(cfg, loop_hz)
        outs = [self.scratch(sl, (n,)) for sl in SLOT_MUX]
        self.api.check(self.api.control_mux(self._h, C.byref(mc), device_ptr(mode), *[device_ptr(a) for a in usr], *[device_ptr(a) for a in ai],
                                            *[device_ptr(o) for o in outs], n), "control_mux")
        return tuple(outs)

    # -- the one exchange of the multi-GPU path (trs_comm_* / trs_allgather_returns: RCCL behind the C ABI) ----------------
    def comm_unique_id(self):
        """Rank 0: the 128-byte id every rank passes to ``comm_init`` (hand it over by any host channel)."""
        buf = C.create_string_buffer(_ffi.COMM_ID_BYTES)
        self.api.check(self.api.comm_get_unique_id(buf), "comm_get_unique_id")
        return buf.raw

    def comm_init(self, rank, world, unique_id=None):
        uid = None if unique_id is None else C.create_string_buffer(bytes(unique_id), _ffi.COMM_ID_BYTES)
        self.api.check(self.api.comm_init(self._h, int(rank), int(world), uid), "comm_init")
        self._comm_world = int(world)

    def comm_destroy(self):
        self.api.check(self.api.comm_destroy(self._h), "comm_destroy")
        self._comm_world = 0

    def allgather_returns(self):
        """``ep_return`` of every env of every shard, ordered by rank, as a fresh ``float32[world * n_envs]`` host array."""
        out = np.empty(self._comm_world * self.n, np.float32)
        self.api.check(self.api.allgather_returns(self._h, None, out.ctypes.data), "allgather_returns")
        return out

    def allgather_returns_device(self):
        """Same, device resident: a zero-copy handle on the handle-owned buffer (the gather is queued on the env's stream;
        the handle is handed out after a host synchronisation)."""
        ptr = C.c_void_p()
        self.api.check(self.api.allgather_returns(self._h, C.byref(ptr), None), "allgather_returns")
        self.sync()
        return _DevicePtr(ptr.value, (self._comm_world * self.n,), np.float32, self)

    # -- timing (HIP events on the handle's stream) -------------------------------------------
    def event_record(self, slot):
        self.api.check(self.api.event_record(self._h, int(slot)), "event_record")

    def event_elapsed_ms(self, a, b):
        ms = C.c_float()
        self.api.check(self.api.event_elapsed_ms(self._h, int(a), int(b), C.byref(ms)), "event_elapsed_ms")
        return float(ms.value)
