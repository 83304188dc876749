"""``DeviceDataset`` — a collected training set that stays uint8 on the GPU and hands out shuffled minibatches (``trs_sample_batch``,
include/trsim_spec.h "training minibatches"): the reference's ``DataLoader.load`` split, shuffle and batch (``components/keras_train.py:33-69``)
without the float32 copy of the whole set and without a byte crossing to the host.  Made by ``BatchedEnv.dataset``."""
import ctypes as C
import math

import numpy as np

from . import _ffi

_TORCH_DTYPES = {"float32": "float32", "float16": "float16", "uint8": "uint8"}


def _ptr(t):
    return int(t.data_ptr()) or None


_HOST_API = []


def _host_api():
    """The library's function table for the calls that need no device and no handle (opened once)."""
    if not _HOST_API:
        _HOST_API.append(_ffi.load_hip_library())
    return _HOST_API[0]


class Augment:
    """Mirror and colour jitter of a training minibatch, applied inside the gather (``trs_sample_batch_aug``; include/trsim_spec.h, "training
    minibatches, augmentation").  ``mirror``: the probability that a record is mirrored left to right, its steering label negated.  ``gain`` in
    [0, 1) and ``bias`` in [0, 255]: the record is lit again by the scene-lighting rule with ``gain_c = 1 + f * gain`` and ``bias_c = f * bias``,
    ``f`` drawn from [-1, 1) — one pair for the three channels, or with ``per_channel`` one per channel.  The draws are keyed by ``(seed, epoch,
    record number)``: reproducible, and readable on the host (``DeviceDataset.augmentation``).  The library's own refusals validate the values
    (``trs_loader_augment``: host arithmetic, no GPU); the one about the ``full_house`` loader is made where a dataset is known."""

    __slots__ = ("mirror", "gain", "bias", "per_channel", "seed")

    def __init__(self, mirror=0.0, gain=0.0, bias=0.0, per_channel=False, seed=0, _api=None):
        for name, value in (("mirror", float(mirror)), ("gain", float(gain)), ("bias", float(bias)), ("per_channel", bool(per_channel)), ("seed", int(seed))):
            object.__setattr__(self, name, value)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64)")
        api = _api if _api is not None else _host_api()
        cfg = _ffi.TrsLoaderConfig()
        api.default_loader_config(C.byref(cfg))
        if api.loader_augment(C.byref(cfg), C.byref(self.config(api)), 0, 0, 0, 0, None, None, None) != 0:
            raise ValueError((api.last_error() or b"").decode())

    def __setattr__(self, name, value):
        raise AttributeError("an Augment is a value: make another one")

    def __repr__(self):
        return f"Augment(mirror={self.mirror}, gain={self.gain}, bias={self.bias}, per_channel={self.per_channel}, seed={self.seed})"

    def __eq__(self, other):
        return isinstance(other, Augment) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))

    def config(self, api):
        a = _ffi.TrsAugmentConfig()
        api.default_augment_config(C.byref(a))
        a.mirror_prob, a.gain_amp, a.bias_amp, a.per_channel, a.seed = self.mirror, self.gain, self.bias, int(self.per_channel), self.seed
        return a


class DeviceDataset:
    """``frames uint8[capacity, H, W, 3]`` (``None`` for a physics-only set) and ``rows float32[capacity, 8]`` (``_ffi.EXPERT_ROW``) in torch device
    storage the dataset owns, of which the first ``len(self)`` records are filled.  ``sigma = perm(mix(seed), n, .)`` splits them: ``n_train =
    floor(split * n)`` training records, the rest validation; every epoch of a split has its own order.  All of it is a function of ``(seed, n,
    n_train, epoch, split, position)``: the same everywhere, reproducible, and readable on the host (``order``)."""

    def __init__(self, env, loader="speed_ctl", label="expert", split=0.8, seed=0, capacity=0, with_frames=True):
        if not getattr(env.api, "has_loader", False):
            raise RuntimeError("this library has no minibatch loader (trs_sample_batch): HIP library only")
        for name, value, table in (("loader", loader, _ffi.LOADER_TYPES), ("label", label, _ffi.LOADER_LABELS)):
            if value not in table:
                raise ValueError(f"{name} must be one of {sorted(table)}")
        if not 0.0 <= float(split) <= 1.0:
            raise ValueError("split must lie in [0, 1]")
        import torch
        self.torch = torch
        self.env, self.loader, self.label, self.split, self.seed = env, loader, label, float(split), int(seed)
        self.device = torch.device(f"cuda:{env.device}")
        self.n = 0
        self.with_frames = bool(with_frames)
        self.frames = torch.empty((0, env.H, env.W, 3), dtype=torch.uint8, device=self.device) if self.with_frames else None
        self.rows = torch.empty((0, 8), dtype=torch.float32, device=self.device)
        self._reserve(int(capacity))

    # -- storage ------------------------------------------------------------------------------------------------------------------
    @property
    def capacity(self):
        return int(self.rows.shape[0])

    def _reserve(self, capacity):
        if capacity <= self.capacity:
            return
        torch = self.torch
        rows = torch.empty((capacity, 8), dtype=torch.float32, device=self.device)
        rows[:self.n].copy_(self.rows[:self.n])
        self.rows = rows
        if self.with_frames:
            frames = torch.empty((capacity, self.env.H, self.env.W, 3), dtype=torch.uint8, device=self.device)
            frames[:self.n].copy_(self.frames[:self.n])
            self.frames = frames

    def _torch_stream(self):
        return self.torch.cuda.current_stream(self.device)

    def _env_after_torch(self, stream=None):
        """Work queued on the env's stream from here on waits for what ``stream`` (default: torch's current stream) holds so far."""
        s = self._torch_stream() if stream is None else stream
        self.env.api.check(self.env.api.stream_wait_external(self.env._h, _ffi_stream(s)), "stream_wait_external")

    def _torch_after_env(self, stream=None):
        s = self._torch_stream() if stream is None else stream
        self.env.api.check(self.env.api.stream_signal_external(self.env._h, _ffi_stream(s)), "stream_signal_external")

    def append(self, frames, rows, jpeg_quality=None):
        """Copy another collection in (device handles as ``BatchedEnv.collect`` returns them, valid only until the next ``collect``; torch tensors
        and host arrays are taken too).  The split is re-derived from the new ``len(self)``: ``n_train = floor(split * n)``, and sigma is a
        permutation of the new ``n``.  ``jpeg_quality``: the new frames go through ``device_jpeg_roundtrip`` once, so that the set holds what a tub's
        files would have given; a quality outside 1..100 (0 included: ``None`` is the only way to ask for no codec) is refused before anything is copied.
        This is DAgger's aggregation: append what ``collect(driver="pilot", ...)`` gathered with the pilot in the loop, then retrain on the larger set."""
        torch = self.torch
        if jpeg_quality is not None and not 1 <= int(jpeg_quality) <= 100:
            raise ValueError("jpeg_quality must lie in 1..100 (None: no codec)")
        if (frames is not None) != self.with_frames:
            raise ValueError("this dataset was made with frames" if self.with_frames else "this dataset is physics-only: it takes rows alone")
        cai = getattr(rows, "__cuda_array_interface__", None)
        if cai is not None and int(np.prod(cai["shape"], dtype=np.int64)) == 0:
            return self                                               # a collection that captured nothing
        with torch.cuda.device(self.device):
            self._torch_after_env()                                   # the handles were written on the env's stream
            r = torch.as_tensor(rows, device=self.device).reshape(-1, 8)
            if r.dtype != torch.float32:
                raise ValueError("rows must be float32[n, 8]")
            k = int(r.shape[0])
            f = None
            if self.with_frames:
                f = torch.as_tensor(frames, device=self.device)
                if f.dtype != torch.uint8 or tuple(f.shape) != (k, self.env.H, self.env.W, 3):
                    raise ValueError(f"frames must be uint8[{k}, {self.env.H}, {self.env.W}, 3]: one frame per row")
            if self.n + k > 2 ** 31 - 1:
                raise ValueError("a set holds at most 2^31 - 1 records")
            if self.n + k > self.capacity:
                self._reserve(max(self.n + k, 2 * self.capacity))
            self.rows[self.n:self.n + k].copy_(r)
            if f is not None:
                self.frames[self.n:self.n + k].copy_(f)
                if jpeg_quality is not None:
                    self._roundtrip(self.n, k, int(jpeg_quality))
            self._env_after_torch()                                   # the env's gathers read what torch's stream has just copied
        self.n += k
        return self

    def _roundtrip(self, start, count, quality, chunk=1024):
        """codec(frame, quality) over frames[start : start + count], in place through a bounce buffer (the codec does not work in place)."""
        torch = self.torch
        bounce = torch.empty((min(chunk, count), self.env.H, self.env.W, 3), dtype=torch.uint8, device=self.device)
        for a in range(start, start + count, chunk):
            m = min(chunk, start + count - a)
            self._env_after_torch()
            self.env.device_jpeg_roundtrip(self.frames[a:a + m], quality, d_dst=bounce, n_images=m)
            self._torch_after_env()
            self.frames[a:a + m].copy_(bounce[:m])

    # -- the split and the order ----------------------------------------------------------------------------------------------------
    def __len__(self):
        return self.n

    @property
    def n_train(self):
        return int(math.floor(self.split * self.n))                  # binary64, as sklearn's train_test_split computes it for train_size = split

    @property
    def n_val(self):
        return self.n - self.n_train

    def _n_split(self, split):
        if split not in _ffi.LOADER_SPLITS:
            raise ValueError("split must be 'train' or 'val'")
        return self.n_train if split == "train" else self.n_val

    def config(self, layout="nchw", dtype="float32"):
        if layout not in _ffi.LOADER_LAYOUTS or dtype not in _ffi.LOADER_DTYPES:
            raise ValueError(f"layout must be one of {sorted(_ffi.LOADER_LAYOUTS)} and dtype one of {sorted(_ffi.LOADER_DTYPES)}")
        c = _ffi.TrsLoaderConfig()
        self.env.api.default_loader_config(C.byref(c))
        c.loader, c.label = _ffi.LOADER_TYPES[self.loader], _ffi.LOADER_LABELS[self.label]
        c.layout, c.dtype = _ffi.LOADER_LAYOUTS[layout], _ffi.LOADER_DTYPES[dtype]
        c.n_records, c.n_train, c.seed = self.n, self.n_train, self.seed
        return c

    def order(self, split="train", epoch=0):
        """The record numbers of an epoch of a split in the order its batches hold them (``trs_loader_order``: host arithmetic, no GPU work)."""
        out = np.empty(self._n_split(split), np.int32)
        c = self.config("nhwc")
        self.env.api.check(self.env.api.loader_order(C.byref(c), _ffi.LOADER_SPLITS[split], int(epoch), 0, out.size, out.ctypes.data), "loader_order")
        return out

    # -- minibatches ------------------------------------------------------------------------------------------------------------------
    def _buffers(self, batch_size, layout, dtype):
        torch = self.torch
        H, W = self.env.H, self.env.W
        shape = (batch_size, 3, H, W) if layout == "nchw" else (batch_size, H, W, 3)
        images = torch.empty(shape, dtype=getattr(torch, _TORCH_DTYPES[dtype]), device=self.device) if self.with_frames else None
        feats = torch.empty((batch_size, _ffi.LOADER_FEATURES[self.loader]), dtype=torch.float32, device=self.device)
        labels = torch.empty((batch_size, 2), dtype=torch.float32, device=self.device)
        index = torch.empty((batch_size,), dtype=torch.int32, device=self.device)
        return images, feats, labels, index

    def augmentation(self, augment, split="train", epoch=0, first=0, count=None):
        """What ``batches(..., augment=augment)`` does to positions ``first .. first + count - 1`` of an epoch of a split (``count=None``: to the end
        of the split): ``(index int32[count], mirror bool[count], params float32[count, 8])``, the record numbers, the mirror flags and ``{gR gG gB 0
        bR bG bB 0}`` per record (``trs_loader_augment``: host arithmetic, no GPU work)."""
        count = self._n_split(split) - int(first) if count is None else int(count)
        index, mirror, params = np.empty(max(count, 0), np.int32), np.empty(max(count, 0), np.uint8), np.empty((max(count, 0), 8), np.float32)
        c, a = self.config("nhwc"), augment.config(self.env.api)
        self.env.api.check(self.env.api.loader_augment(C.byref(c), C.byref(a), _ffi.LOADER_SPLITS[split], int(epoch), int(first), count, index.ctypes.data,
                                                       mirror.ctypes.data, params.ctypes.data), "loader_augment")
        return index, mirror.astype(bool), params

    def sample(self, cfg, split, epoch, first, batch, images, feats, labels, index=None, augment=None):
        """One ``trs_sample_batch`` (``augment``: one ``trs_sample_batch_aug``) into torch tensors, asynchronous on the env's stream."""
        if augment is not None:
            self.env.api.check(self.env.api.sample_batch_aug(
                self.env._h, C.byref(cfg), C.byref(augment.config(self.env.api)), _ptr(self.frames) if self.with_frames else None, _ptr(self.rows),
                _ffi.LOADER_SPLITS[split], int(epoch), int(first), int(batch), None if images is None else _ptr(images),
                _ptr(feats) if feats.numel() else None, _ptr(labels), None if index is None else _ptr(index)), "sample_batch_aug")
            return
        self.env.api.check(self.env.api.sample_batch(
            self.env._h, C.byref(cfg), _ptr(self.frames) if self.with_frames else None, _ptr(self.rows), _ffi.LOADER_SPLITS[split], int(epoch), int(first),
            int(batch), None if images is None else _ptr(images), _ptr(feats) if feats.numel() else None, _ptr(labels), None if index is None else _ptr(index)),
            "sample_batch")

    def batches(self, batch_size, epoch, split="train", layout="nchw", dtype="float32", stream=None, augment=None):
        """Iterator over the ``floor(n_split / batch_size)`` minibatches of an epoch (``drop_remainder``): ``(images, features, labels)`` torch
        tensors — ``images`` in ``layout`` / ``dtype`` (``None`` for a physics-only set), ``features float32[B, F]`` (F = 0 for the loaders without
        features), ``labels float32[B, 2]``.  Three sets of buffers rotate: batch t + 1 is gathered while t is consumed, and the request for batch t + 1
        writes the buffers of batch t - 1, so a yielded batch is valid until the next but one is requested (batch t may be held, on the device or
        read from the host, across the request for t + 1).  Ordering as for ``device_array``: with ``stream=`` (the CONSUMER's stream) that stream
        waits for the gather and the host does not; otherwise the host waits for each batch.  A gather waits for the work the consumer's stream held
        when it was launched, i.e. for everything queued on a batch before the next is requested.  The buffers are allocated on the consumer's
        stream, so torch's allocator hands them on only behind that stream's reads.  ``augment``: an ``Augment`` — the records of this split are
        mirrored and lit again inside the gather, by draws keyed with ``epoch`` and the record number (``augmentation`` reports them); pass it for
        ``"train"`` only, validation measures the frames as collected.  ``None``: the plain gather."""
        torch = self.torch
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError("augment must be an Augment or None")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size >= 1 is required")
        cfg = self.config(layout, dtype)
        n_batches = self._n_split(split) // batch_size
        consumer = self._torch_stream() if stream is None else stream
        if not hasattr(consumer, "cuda_stream"):                     # a raw stream pointer, as device_array takes it
            consumer = torch.cuda.ExternalStream(int(consumer), device=self.device)
        with torch.cuda.stream(consumer):
            bufs = [self._buffers(batch_size, layout, dtype) for _ in range(min(3, n_batches))]

        def gather(t):
            self._env_after_torch(stream)
            self.sample(cfg, split, epoch, t * batch_size, batch_size, *bufs[t % 3], augment=augment)

        if n_batches:
            gather(0)
        for t in range(n_batches):
            if stream is not None:
                self._torch_after_env(stream)                        # the consumer's stream waits for gather(t) alone: t + 1 is not queued yet
            else:
                self.env.sync()
            if t + 1 < n_batches:
                gather(t + 1)                                        # into the buffers of batch t - 2: t - 1 stays as it was handed out
            yield bufs[t % 3][:3]

    def pilot_loss(self, split="val", batch_size=None, epoch=0):
        """Mean squared error of the loaded HIP pilot (``pilot_load``; ``trs_pilot_forward_ex`` on uint8 minibatches) against the labels, over the
        ``floor(n_split / batch_size)`` batches of the split: the ``val_loss`` the reference's ``ModelCheckpoint`` watches
        (``components/keras_train.py:406-408``), of the fp16 pilot as it will drive.  ``batch_size``: at most ``n_envs``, what the pilot's buffers hold
        (``None``: ``n_envs``, or the whole split when that is smaller).  Never augmented: the loss is of the frames as collected.  Returns a Python float."""
        if not self.with_frames:
            raise RuntimeError("a physics-only set has no frames for the pilot")
        torch = self.torch
        batch_size = max(min(self.env.n, self._n_split(split)), 1) if batch_size is None else int(batch_size)
        if not 1 <= batch_size <= self.env.n:
            raise ValueError(f"batch_size must lie in [1, n_envs = {self.env.n}]: the pilot runs at most n_envs frames per call")
        n_batches = self._n_split(split) // batch_size
        if n_batches < 1:
            raise ValueError(f"the {split!r} split holds {self._n_split(split)} records: no batch of {batch_size}")
        total = n_batches * batch_size
        cfg = self.config("nhwc", "uint8")
        with torch.cuda.device(self.device):
            images = torch.empty((batch_size, self.env.H, self.env.W, 3), dtype=torch.uint8, device=self.device)
            feats = torch.empty((batch_size, _ffi.LOADER_FEATURES[self.loader]), dtype=torch.float32, device=self.device)
            labels = torch.empty((total, 2), dtype=torch.float32, device=self.device)
            out = torch.empty((total, 2), dtype=torch.float32, device=self.device)
            # the pilot takes 'gym/speed' (it divides by 20 inside) and 'loc/segment' as they were recorded, one value per frame; the model types
            # without those inputs do not read them
            idx = torch.as_tensor(self.order(split, epoch)[:total].astype(np.int64), device=self.device)
            speed, segment = self.rows[idx, 4].contiguous(), self.rows[idx, 6].contiguous()
            self._env_after_torch()
            for t in range(n_batches):
                a = t * batch_size
                self.sample(cfg, split, epoch, a, batch_size, images, feats, labels[a:a + batch_size])
                self.env.api.check(self.env.api.pilot_forward_ex(self.env._h, _ptr(images), _ptr(speed[a:]), _ptr(segment[a:]), batch_size, _ptr(out[a:a + batch_size])),
                                   "pilot_forward_ex")
            self._torch_after_env()
            return float(torch.mean((out.double() - labels.double()) ** 2).item())

    def fit_tail(self, epochs, batch_size, augment=None, patience=None, val_batch_size=None, convs=None, **adam):
        """Train the loaded pilot's dense tail on this set, on the device (``trs_pilot_train_step``; include/trsim_spec.h, "training the pilot's
        tail"): dense1 .. output_layer move by Adam on 'mse'.  ``convs``: names among ``"conv4"`` .. ``"conv7"`` that move with them
        ("training the pilot's last convolutions"); ``None``: every convolution stays as loaded.  conv1 .. conv3 always do.  What ``model.fit`` is to the reference's trainer
        for a model continued from a saved one (``components/keras_train.py:376,400-411``), without a second copy of the network in a framework:
        per epoch the uint8 NHWC batches of ``batches(batch_size, epoch, "train", augment=augment)`` go into one training step each, then
        ``pilot_loss("val", val_batch_size)`` is taken on the fp16 pilot as it drives.  The best epoch's weights are kept
        (``ModelCheckpoint(save_best_only=True)``), ``patience`` epochs without a better validation loss stop the run (``None``: all ``epochs``),
        and at the end the best weights are loaded into the handle.  ``adam``: ``lr``, ``beta1``, ``beta2``, ``eps``, ``layers`` of
        ``pilot_train_begin``, and its ``dropout`` (a rate; the reference's is 0.1), ``dropout_sites``, ``dropout_seed``: training-mode dropout
        behind conv7 and the hidden dense layers ("training the pilot's tail, dropout"), in the training steps alone — ``train_loss`` is the
        dropped network's, ``val_loss`` is taken without dropout, as Keras reports them.  Returns the list of ``(train_loss, val_loss)`` per epoch
        run, ``train_loss`` the mean of the batches' losses.
        With a 28-array pilot loaded (``cnn_2d_speed_as_feature``) the set must come from the ``speed_feature`` loader: each batch's feature, speed / 20,
        goes into the step with its frames, and feature1 .. feature3 move with the tail ("training the pilot's tail, side branch"; ``layers`` also takes
        their names); the best epoch's 14 arrays are kept and restored.
        Not here: dropout behind conv1 .. conv6, training conv1 .. conv3, ``cnn_2d_full_house``."""
        if not self.with_frames:
            raise RuntimeError("a physics-only set has no frames for the pilot")
        torch, env = self.torch, self.env
        side = len(getattr(env, "_pilot_arrays", None) or ()) == 28
        if side and self.loader != "speed_feature":
            raise ValueError(f"a 28-array pilot (cnn_2d_speed_as_feature) trains on the 'speed_feature' loader's batches: this set's loader is {self.loader!r}")
        epochs, batch_size = int(epochs), int(batch_size)
        if epochs < 1 or not 1 <= batch_size <= env.n:
            raise ValueError(f"epochs >= 1 and batch_size in [1, n_envs = {env.n}] are required")
        if self.n_train // batch_size < 1:
            raise ValueError(f"the 'train' split holds {self.n_train} records: no batch of {batch_size}")
        if patience is not None and int(patience) < 1:
            raise ValueError("patience >= 1 is required (None: no early stop)")
        history, best, best_val, since = [], None, math.inf, 0
        env.pilot_train_begin(convs=convs, **adam)
        try:
            with torch.cuda.device(self.device):
                stream = self._torch_stream()
                n_batches = self.n_train // batch_size
                losses = torch.zeros((n_batches,), dtype=torch.float32, device=self.device)
                for epoch in range(epochs):
                    for t, (images, feats, labels) in enumerate(self.batches(batch_size, epoch, "train", layout="nhwc", dtype="uint8", stream=stream, augment=augment)):
                        # the gather and the step run on the env's stream, one behind the other: the torch stream's wait inside batches() is all the order needed
                        env.pilot_train_step(images, labels, batch_size, loss=losses[t:], features=feats if side else None)
                    self._torch_after_env()
                    train_loss = float(losses.double().mean().item())
                    val_loss = self.pilot_loss("val", val_batch_size)
                    history.append((train_loss, val_loss))
                    if val_loss < best_val:
                        best_val, since = val_loss, 0
                        best = (env.pilot_train_weights()[0], env.pilot_train_conv_weights() if convs is not None else None)
                    else:
                        since += 1
                        if patience is not None and since >= int(patience):
                            break
        finally:
            env.pilot_train_end()
        if best is not None:
            arrs = env.pilot_weights()
            arrs[14:14 + len(best[0])] = best[0]
            if best[1] is not None:
                arrs[6:14] = best[1]
            env.pilot_load(arrs)
        return history

    def fit(self, epochs, batch_size, convs=("conv4", "conv5", "conv6", "conv7"), **kwargs):
        """``fit_tail`` under the name of what it does by default here: dense1 .. output_layer and the convolutions named in ``convs`` (conv4 ..
        conv7 unless told otherwise) are trained; conv1 .. conv3 stay as loaded.  ``dropout=0.1`` adds the reference's dropout behind conv7 and the hidden dense
        layers (``fit_tail``)."""
        return self.fit_tail(epochs, batch_size, convs=convs, **kwargs)


def _ffi_stream(stream):
    """A torch stream as the pointer value the C ABI takes (0, the legacy default stream, as NULL)."""
    return int(getattr(stream, "cuda_stream", stream)) or None
