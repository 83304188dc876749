"""ctypes binding of the C ABI declared in ``include/trsim.h``.

This is the reference-side stub a maintainer of Triton-Racer-Sim would add (the reference is
Python, so its FFI is ctypes).  ``bind(cdll, prefix)`` types every entry
point; ``load_hip_library()`` opens the in-tree HIP build and FAILS LOUDLY when it is missing —
there is no CPU fallback in the product.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_HERE, "csrc", "libtrsim.so")


class TrsConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_envs", C.c_int32), ("env_id_base", C.c_int32),
        ("img_h", C.c_int32), ("img_w", C.c_int32),
        ("render", C.c_int32), ("auto_reset", C.c_int32), ("depth", C.c_int32),
        ("seed", C.c_uint64),
        ("dt", C.c_float), ("max_steer", C.c_float), ("inv_wheelbase", C.c_float), ("accel_max", C.c_float),
        ("drag_lin", C.c_float), ("roll_res", C.c_float), ("brake_max", C.c_float),
        ("v_max", C.c_float), ("v_rev_max", C.c_float), ("offtrack_cte", C.c_float),
        ("offtrack_penalty", C.c_float), ("cam_fwd", C.c_float),
        ("road_half", C.c_double), ("edge_half", C.c_double), ("centre_half", C.c_double),
        ("dash_period", C.c_double), ("dash_on", C.c_double), ("map_margin", C.c_double),
        ("fov_v_deg", C.c_double), ("cam_h", C.c_double), ("cam_pitch_deg", C.c_double), ("z_far", C.c_double),
    ]


class TrsStateView(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32), ("n_points", C.c_int32),
        ("img", C.c_void_p),
        ("pos_x", C.c_void_p), ("pos_y", C.c_void_p), ("pos_z", C.c_void_p), ("speed", C.c_void_p), ("cte", C.c_void_p),
        ("yaw", C.c_void_p), ("vel", C.c_void_p), ("seg_idx", C.c_void_p),
        ("ep_return", C.c_void_p), ("last_return", C.c_void_p), ("ep_len", C.c_void_p), ("done", C.c_void_p),
        ("step_count", C.c_uint64),
        ("depth", C.c_void_p),
    ]


class TrsObsView(C.Structure):
    """``trs_obs_view`` (include/trsim.h): what the cars are told after the last step, as device pointers (``trs_get_observation``)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_envs", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32),
        ("img", C.c_void_p), ("depth", C.c_void_p),
        ("pos_x", C.c_void_p), ("pos_y", C.c_void_p), ("pos_z", C.c_void_p), ("speed", C.c_void_p), ("cte", C.c_void_p),
        ("seg_idx", C.c_void_p), ("arrived", C.c_void_p),
    ]


class TrsMapInfo(C.Structure):
    _fields_ = [
        ("map_w", C.c_int32), ("map_h", C.c_int32), ("map_words", C.c_int32),
        ("cell", C.c_double), ("x0", C.c_double), ("z0", C.c_double),
        ("n_points", C.c_int32), ("lds_bytes", C.c_int32),
    ]


class TrsPreConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("dynamic_brightness", C.c_int32), ("brightness_baseline", C.c_double),
        ("contrast_ratio", C.c_float), ("contrast_offset", C.c_float),
        ("color_filter_enabled", C.c_int32), ("n_filters", C.c_int32),
        ("hsv_lo", (C.c_uint8 * 3) * 4), ("hsv_hi", (C.c_uint8 * 3) * 4), ("dst_channel", C.c_int32 * 4),
        ("edge_detection_enabled", C.c_int32), ("edge_threshold_a", C.c_int32), ("edge_threshold_b", C.c_int32),
        ("edge_dst_channel", C.c_int32),
    ]


# selectors of trs_copy_to_host: name -> (enum value, numpy dtype string, per-env? shape tag)
FIELDS = {
    "img": 0, "pos_x": 1, "pos_y": 2, "pos_z": 3, "speed": 4, "cte": 5, "yaw": 6, "vel": 7,
    "seg_idx": 8, "ep_return": 9, "last_return": 10, "ep_len": 11, "done": 12,
    "map": 13, "rowtab": 14, "palette": 15, "tangent": 16, "steer_filt": 17, "stats": 18, "depth": 19, "rowdepth": 20,
    "ctl_steer": 21, "ctl_thr": 22, "ctl_brk": 23, "dpitch": 24, "lens_table": 25, "lens_palette": 26,
}

# every symbol include/trsim.h declares (suffix after the prefix)
SYMBOLS = [
    "default_config", "create", "destroy", "load_track", "reset", "step", "step_host", "step_synthetic", "step_sequence", "step_sequence_host",
    "set_step_mode", "get_step_mode", "quiesce", "step_wait", "get_state", "copy_to_host", "fetch_outputs", "set_pose", "locate", "map_info_get", "sync", "event_record",
    "event_elapsed_ms", "device_count", "last_error",
    "default_pre_config", "preprocess", "preprocess_host", "set_frame_filter", "normalize", "normalize_host",
    "driver_assist", "driver_assist_host",
    "default_mux_config", "control_mux", "control_mux_host", "control_mux_reset",
    "comm_get_unique_id", "comm_init", "comm_destroy", "allgather_returns", "stream_wait_external", "stream_signal_external",
    "scratch", "upload", "counters",
]


class TrsCamera(C.Structure):
    """``trs_camera`` (include/trsim.h): the lens camera of ``trs_set_camera``."""
    _fields_ = [("struct_size", C.c_uint32), ("fish_eye_x", C.c_double), ("fish_eye_y", C.c_double), ("offset_x", C.c_double)]


class TrsMuxConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("throttle_lock_enabled", C.c_int32), ("throttle_lock_value", C.c_float), ("throttle_lock_ticks", C.c_int32),
        ("steering_lock_enabled", C.c_int32), ("steering_lock_value", C.c_float), ("steering_lock_ticks", C.c_int32),
    ]


class TrsPilotConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("spd_ctl_threshold", C.c_float), ("spd_ctl_break", C.c_int32),
        ("spd_ctl_reverse_multiplier", C.c_float), ("spd_ctl_break_multiplier", C.c_float),
        ("smooth_steering_enabled", C.c_int32), ("smooth_steering_threshold", C.c_float),
        ("model_type", C.c_int32),
    ]


class TrsPilotTuning(C.Structure):
    """``trs_pilot_tuning`` (include/trsim.h): kernel choices of ``trs_pilot_load``; tests and measurements only."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("no_fuse", C.c_int32), ("fuse_band_r2", C.c_int32), ("fuse_wsplit_max", C.c_int32), ("fuse_roll", C.c_int32),
        ("span_layers_mask", C.c_int32), ("frame5", C.c_int32), ("frame_layers_mask", C.c_int32), ("chain_layers", C.c_int32), ("dense", C.c_int32), ("ksplit", C.c_int32),
    ]


class TrsExpertConfig(C.Structure):
    """``trs_expert_config`` (include/trsim.h): the scripted expert of ``trs_set_expert``."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("look", C.c_int32), ("k_cte", C.c_float), ("k_head", C.c_float), ("thr_hi", C.c_float), ("thr_lo", C.c_float),
        ("target_speed", C.c_float), ("brake_over", C.c_float), ("brake_val", C.c_float), ("alpha", C.c_float), ("sigma", C.c_float),
        ("seed", C.c_uint64),
    ]


class TrsExpertCapture(C.Structure):
    """``trs_expert_capture`` (include/trsim.h): where ``trs_step_expert`` puts the records of the ticks it captures."""
    _fields_ = [("struct_size", C.c_uint32), ("every", C.c_int32), ("skip", C.c_int32), ("capacity", C.c_int32), ("d_frames", C.c_void_p), ("d_rows", C.c_void_p)]


class TrsDaggerConfig(C.Structure):
    """``trs_dagger_config`` (include/trsim.h): the gate of ``trs_step_dagger``."""
    _fields_ = [("struct_size", C.c_uint32), ("beta", C.c_float), ("hold", C.c_int32), ("expert_speed", C.c_int32), ("seed", C.c_uint64)]


class TrsLoaderConfig(C.Structure):
    """``trs_loader_config`` (include/trsim.h): which minibatches ``trs_sample_batch`` gathers from a collected set."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("loader", C.c_int32), ("label", C.c_int32), ("layout", C.c_int32), ("dtype", C.c_int32),
        ("n_records", C.c_int32), ("n_train", C.c_int32), ("seed", C.c_uint64),
    ]


class TrsAugmentConfig(C.Structure):
    """``trs_augment_config`` (include/trsim.h): the mirror and colour jitter ``trs_sample_batch_aug`` applies inside the gather."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("mirror_prob", C.c_float), ("gain_amp", C.c_float), ("bias_amp", C.c_float), ("per_channel", C.c_int32),
        ("seed", C.c_uint64),
    ]


class TrsTrainConfig(C.Structure):
    """``trs_train_config`` (include/trsim.h): Adam's constants and the layers ``trs_pilot_train_step`` moves."""
    _fields_ = [("struct_size", C.c_uint32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("train_mask", C.c_uint32)]


class TrsDropoutConfig(C.Structure):
    """``trs_dropout_config`` (include/trsim.h): training-mode dropout behind conv7 (``trs_pilot_train_dropout``)."""
    _fields_ = [("struct_size", C.c_uint32), ("rate", C.c_float), ("sites", C.c_uint32), ("seed", C.c_uint64)]


TRAIN_LAYERS = ("dense1", "dense2", "dense3", "output_layer")           # bit l of trs_train_config.train_mask; their (kernel, bias) pairs are the eight trained arrays
TRAIN_SIDE_LAYERS = TRAIN_LAYERS + ("feature1", "feature2", "feature3")   # a 28-array session: bits 4 .. 6 name the branch's layers; 14 trained arrays
TRAIN_DEBUG = {"out": 0, "z1": 1, "z2": 2, "z3": 3, "delta1": 4, "delta2": 5, "delta3": 6, "delta4": 7, "gw1": 8, "gw2": 9, "gw3": 10, "gw4": 11,
               "gb1": 12, "gb2": 13, "gb3": 14, "gb4": 15, "m": 16, "v": 24, "scale_exp": 32, "loss": 33, "pack1": 34,
               "a1": 36, "a2": 37, "a3": 38}                            # TRS_TRAIN_DBG_* ("m", "v": + the array's number 0..7; 35 is no item)
# TRS_TRAIN_SIDE_* (trs_pilot_train_debug_side): name -> (item, floats per frame, or None for an array's size); "g", "m", "v" take the side array's name
TRAIN_SIDE_DEBUG = {"fin": (0, 1), "y1": (1, 4), "y2": (2, 8), "y3": (3, 16), "dy1": (4, 4), "dy2": (5, 8), "dy3": (6, 16), "g": (8, None), "m": (16, None), "v": (24, None)}
TRAIN_SIDE_ARRAYS = {"w1y": (0, 1600), "f1w": (1, 4), "f1b": (2, 4), "f2w": (3, 32), "f2b": (4, 8), "f3w": (5, 128), "f3b": (6, 16)}   # side array -> (number, floats)

LOADER_TYPES = {"speed_ctl": 0, "default": 1, "speed_feature": 2, "full_house": 3}   # TRS_LOADER_*; the names of recorder.LOADERS, in the order of TRS_PILOT_*
LOADER_FEATURES = {"speed_ctl": 0, "default": 0, "speed_feature": 1, "full_house": 2}
LOADER_LABELS = {"expert": 0, "applied": 1}                             # TRS_LABEL_*
LOADER_LAYOUTS = {"nhwc": 0, "nchw": 1}                                 # TRS_LAYOUT_*
LOADER_DTYPES = {"float32": 0, "float16": 1, "uint8": 2}                # TRS_DTYPE_*
LOADER_SPLITS = {"train": 0, "val": 1}                                  # TRS_SPLIT_*

EXPERT_ROW = ("steering", "throttle", "breaking", "applied_steering", "speed", "cte", "segment", "done")   # a record row of trs_step_expert's capture
DAGGER_STATS = ("ticks", "expert_ticks", "sum_abs_cte", "max_abs_cte", "sum_abs_steering_diff", "done_ticks")   # a stats row of trs_dagger_stats

COMM_ID_BYTES = 128                                                    # TRS_COMM_ID_BYTES

PILOT_MODEL_TYPES = {"cnn_2d_speed_control": 0, "cnn_2d": 1, "cnn_2d_speed_as_feature": 2, "cnn_2d_full_house": 3}   # TRS_PILOT_*; ModelType values (utils/types.py)

# layer names in the order trs_pilot_load takes their (kernel, bias) pairs (include/trsim.h), per architecture
PILOT_LAYERS = {
    22: ["conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "dense1", "dense2", "dense3", "output_layer"],
    28: ["conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "dense1", "dense2", "dense3", "output_layer", "feature1", "feature2", "feature3"],
    42: ["conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "dense1", "dense2", "dense3", "output_speed", "feature1", "feature2", "feature3",
         "current_spd_1", "current_spd_2", "current_spd_3", "dense4", "dense5", "dense6", "out_steering"],
}
PILOT_ARRAYS_OF_TYPE = {"cnn_2d_speed_control": 22, "cnn_2d": 22, "cnn_2d_speed_as_feature": 28, "cnn_2d_full_house": 42}


# HIP library only: the lens camera (trs_set_camera) has no twin in the C oracle — its checker is the restatement of include/trsim_spec.h
# ("lens camera") in tests/test_lens_tables_cpu.py and tests/test_lens_gpu.py, and oracle/ stays as it is
LENS_SYMBOLS = ["default_camera", "set_camera", "get_camera"]
# HIP library only: scene lighting (trs_set_lighting) has no twin in the C oracle either — its checker is the oracle's unlit frame with the rule of
# include/trsim_spec.h ("scene lighting") applied in numpy (tests/test_lighting_cpu.py, tests/test_lighting_gpu.py)
LIGHT_SYMBOLS = ["set_lighting", "set_lighting_host"]
# HIP library only: observation latency (trs_set_latency) is a view on the truth the oracle already checks — its checker is the history of oracle records
# with the rule of include/trsim_spec.h ("observation latency") applied in Python (tests/test_latency_cpu.py, tests/test_latency_gpu.py)
LATENCY_SYMBOLS = ["set_latency", "get_latency", "get_observation", "fetch_observation"]
# HIP library only: the tub image encoder (trs_encode_jpeg) — its checker is the numpy restatement of include/trsim_spec.h ("tub image (JPEG)") in
# tests/test_jpeg_cpu.py, itself pinned to Pillow's files byte for byte (tests/test_jpeg_gpu.py compares the kernel's files with it)
JPEG_SYMBOLS = ["jpeg_header_bytes", "encode_jpeg", "encode_jpeg_host"]
# HIP library only: the tub image decoder (trs_decode_jpeg) — its checker is the restatement of include/trsim_spec.h ("tub image (JPEG), decoding") in
# tests/test_jpeg_decode_cpu.py, itself pinned to Pillow's decoder byte for byte (tests/test_jpeg_decode_gpu.py compares the kernel's frames with it)
JPEG_DECODE_SYMBOLS = ["decode_jpeg", "decode_jpeg_host"]
# HIP library only: the camera codec (trs_jpeg_roundtrip, trs_set_camera_codec) — its checker is the restatement of include/trsim_spec.h ("camera codec
# (JPEG round trip)") in tests/test_jpeg_codec_cpu.py, itself pinned to decode(encode()) of the two restatements above and to Pillow's save and open
JPEG_CODEC_SYMBOLS = ["jpeg_roundtrip", "jpeg_roundtrip_host", "set_camera_codec", "get_camera_codec"]
# HIP library only: the scripted expert (trs_set_expert, trs_step_expert) — its checker is the numpy restatement of include/trsim_spec.h ("scripted expert") in
# tests/test_expert_cpu.py, which drives the oracle with it (tests/test_expert_gpu.py compares the kernel with the restatement bit for bit)
EXPERT_SYMBOLS = ["default_expert_config", "set_expert", "expert_act", "step_expert"]
# HIP library only: the training minibatches (trs_sample_batch, trs_loader_order) — their checker is the numpy restatement of include/trsim_spec.h
# ("training minibatches") in tests/test_loader_cpu.py (tests/test_loader_gpu.py compares the kernel with the restatement bit for bit)
LOADER_SYMBOLS = ["default_loader_config", "sample_batch", "loader_order"]
# HIP library only: the augmented minibatches (trs_sample_batch_aug, trs_loader_augment) — their checker is the numpy restatement of include/trsim_spec.h
# ("training minibatches, augmentation") in tests/test_augment_cpu.py (tests/test_augment_gpu.py compares the kernel with the restatement bit for bit)
AUGMENT_SYMBOLS = ["default_augment_config", "sample_batch_aug", "loader_augment"]
# HIP library only: the pilot in the loop with the expert's labels (trs_step_dagger) — its checker is the numpy restatement of include/trsim_spec.h ("pilot
# in the loop with the expert's labels") in tests/test_dagger_cpu.py composed with the existing calls (tests/test_dagger_gpu.py, bit for bit)
DAGGER_SYMBOLS = ["default_dagger_config", "step_dagger", "dagger_stats"]
# HIP library only: training the pilot's tail (trs_pilot_train_*) — its checker is the numpy restatement of include/trsim_spec.h ("training the pilot's
# tail") in tests/test_train_cpu.py, itself checked against torch.autograd in binary64 (tests/test_train_gpu.py compares the kernels with it)
TRAIN_SYMBOLS = ["default_train_config", "pilot_train_begin", "pilot_train_step", "pilot_train_get", "pilot_train_debug", "pilot_train_end"]
# HIP library only: training the pilot's last convolutions (trs_pilot_train_convs) — its checker is the numpy restatement of include/trsim_spec.h
# ("training the pilot's last convolutions") in tests/test_train_conv_cpu.py, itself checked against torch.autograd in binary64
TRAIN_CONV_SYMBOLS = ["pilot_train_convs", "pilot_train_get_convs", "pilot_train_debug_conv"]
# HIP library only: dropout behind conv7 (trs_pilot_train_dropout, trs_train_dropout_keep) — its checker is the numpy restatement of include/trsim_spec.h
# ("training the pilot's tail, dropout") in tests/test_dropout_cpu.py (tests/test_dropout_gpu.py compares the kernels with it, the masks bit for bit)
DROPOUT_SYMBOLS = ["default_dropout_config", "pilot_train_dropout", "train_dropout_keep"]
DROPOUT_SITES = ("x7", "a1", "a2", "a3")                                # bit j of trs_dropout_config.sites; units per frame: F, 100, 50, 25
# HIP library only: training the speed-as-feature pilot (trs_pilot_train_*_ex, trs_pilot_train_debug_side) — its checker is the numpy restatement of
# include/trsim_spec.h ("training the pilot's tail, side branch") in tests/test_train_side_cpu.py, itself checked against torch.autograd in binary64
TRAIN_SIDE_SYMBOLS = ["pilot_train_begin_ex", "pilot_train_step_ex", "pilot_train_get_ex", "pilot_train_debug_side"]
TRAIN_CONV_LAYERS = ("conv4", "conv5", "conv6", "conv7")                # bit j of trs_pilot_train_convs' mask; arrays 6 + 2 j, 7 + 2 j of pilot_load
TRAIN_CONV_DEBUG = {"delta": 0, "gw": 1, "gb": 2, "mw": 3, "vw": 4, "mb": 5, "vb": 6, "scale_exp": 7, "pack": 8}   # TRS_CONV_DBG_*
# HIP library only: the CNN pilot is a floating-point kernel whose checker is a PyTorch fp32 reference, not the C oracle
PILOT_SYMBOLS = ["default_pilot_config", "pilot_load", "pilot_forward", "pilot_forward_host", "pilot_forward_ex", "pilot_forward_host_ex",
                 "pilot_debug_layer", "pilot_range_check", "pilot_act", "step_pilot", "default_pilot_tuning", "pilot_set_tuning"] + TRAIN_SYMBOLS + TRAIN_CONV_SYMBOLS + DROPOUT_SYMBOLS + TRAIN_SIDE_SYMBOLS + LENS_SYMBOLS + LIGHT_SYMBOLS + LATENCY_SYMBOLS + JPEG_SYMBOLS + JPEG_DECODE_SYMBOLS + JPEG_CODEC_SYMBOLS + EXPERT_SYMBOLS + LOADER_SYMBOLS + DAGGER_SYMBOLS + AUGMENT_SYMBOLS
# test hooks of the resident worker: only in csrc/libtrsim_testhooks.so (-DTRS_TEST_HOOKS), never in the product library
HOOK_SYMBOLS = ["resident_debug_lifetime", "resident_debug_abort"]
HIP_TESTHOOKS_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libtrsim_testhooks.so")


class Api:
    """Typed function table of one loaded library (``trs_*`` for HIP, ``trso_*`` for the test oracle)."""

    def __init__(self, cdll, prefix):
        self.cdll, self.prefix = cdll, prefix
        vp, i32, fp, u8p, dp = C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p
        sigs = {
            "default_config": (None, [C.POINTER(TrsConfig)]),
            "create": (i32, [C.POINTER(TrsConfig), i32, C.POINTER(vp)]),
            "destroy": (i32, [vp]),
            "load_track": (i32, [vp, dp, i32]),
            "reset": (i32, [vp, u8p]),
            "step": (i32, [vp, fp, fp, fp, u8p, i32]),
            "step_host": (i32, [vp, fp, fp, fp, u8p, i32]),
            "step_synthetic": (i32, [vp, i32, i32]),
            "step_sequence": (i32, [vp, fp, fp, fp, u8p, i32, i32]),
            "step_sequence_host": (i32, [vp, fp, fp, fp, u8p, i32, i32]),
            "set_step_mode": (i32, [vp, i32, i32]),
            "get_step_mode": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
            "quiesce": (i32, [vp]),
            "step_wait": (i32, [vp, fp, fp, fp, u8p, i32]),
            "get_state": (i32, [vp, C.POINTER(TrsStateView)]),
            "copy_to_host": (i32, [vp, i32, vp, C.c_size_t]),
            "fetch_outputs": (i32, [vp] + [vp] * 8),
            "set_pose": (i32, [vp, fp, fp, fp, fp, fp]),
            "locate": (i32, [vp, dp, i32, vp]),
            "map_info_get": (i32, [vp, C.POINTER(TrsMapInfo)]),
            "sync": (i32, [vp]),
            "event_record": (i32, [vp, i32]),
            "event_elapsed_ms": (i32, [vp, i32, i32, C.POINTER(C.c_float)]),
            "device_count": (i32, [C.POINTER(i32)]),
            "last_error": (C.c_char_p, []),
            "default_pre_config": (None, [C.POINTER(TrsPreConfig)]),
            "preprocess": (i32, [vp, C.POINTER(TrsPreConfig), vp, vp, i32, C.POINTER(vp)]),
            "preprocess_host": (i32, [vp, C.POINTER(TrsPreConfig), vp, vp, i32]),
            "set_frame_filter": (i32, [vp, C.POINTER(TrsPreConfig)]),
            "normalize": (i32, [vp, vp, vp, i32]),
            "normalize_host": (i32, [vp, vp, vp, i32]),
            "driver_assist": (i32, [vp, i32, C.c_double, vp, vp, vp, vp, i32]),
            "driver_assist_host": (i32, [vp, i32, C.c_double, vp, vp, vp, vp, i32]),
            "default_mux_config": (None, [C.POINTER(TrsMuxConfig)]),
            "control_mux": (i32, [vp, C.POINTER(TrsMuxConfig), vp] + [vp] * 9 + [i32]),
            "control_mux_host": (i32, [vp, C.POINTER(TrsMuxConfig), vp] + [vp] * 9 + [i32]),
            "control_mux_reset": (i32, [vp]),
            "comm_get_unique_id": (i32, [vp]),
            "comm_init": (i32, [vp, i32, i32, vp]),
            "comm_destroy": (i32, [vp]),
            "allgather_returns": (i32, [vp, C.POINTER(vp), vp]),
            "stream_wait_external": (i32, [vp, vp]),
            "stream_signal_external": (i32, [vp, vp]),
            "scratch": (i32, [vp, i32, C.c_size_t, C.POINTER(vp)]),
            "upload": (i32, [vp, vp, vp, C.c_size_t]),
            "counters": (i32, [vp, C.POINTER(C.c_uint64 * 4)]),
        }
        pilot = {
            "default_pilot_config": (None, [C.POINTER(TrsPilotConfig)]),
            "pilot_load": (i32, [vp, C.POINTER(C.c_void_p), i32]),
            "pilot_forward": (i32, [vp, vp, i32, vp]),
            "pilot_forward_host": (i32, [vp, vp, i32, vp]),
            "pilot_debug_layer": (i32, [vp, i32, vp, C.c_size_t]),
            "pilot_range_check": (i32, [vp, vp]),
            "pilot_forward_ex": (i32, [vp, vp, vp, vp, i32, vp]),
            "pilot_forward_host_ex": (i32, [vp, vp, vp, vp, i32, vp]),
            "pilot_act": (i32, [vp, C.POINTER(TrsPilotConfig), vp, vp, vp, vp, vp, vp, vp, i32]),
            "step_pilot": (i32, [vp, C.POINTER(TrsPilotConfig), i32]),
            "default_pilot_tuning": (None, [C.POINTER(TrsPilotTuning)]),
            "pilot_set_tuning": (i32, [vp, C.POINTER(TrsPilotTuning)]),
        }
        lens = {
            "default_camera": (None, [C.POINTER(TrsCamera)]),
            "set_camera": (i32, [vp, C.POINTER(TrsCamera)]),
            "get_camera": (i32, [vp, C.POINTER(TrsCamera)]),
        }
        light = {
            "set_lighting": (i32, [vp, vp]),
            "set_lighting_host": (i32, [vp, C.POINTER(C.c_float)]),
        }
        latency = {
            "set_latency": (i32, [vp, vp, i32]),
            "get_latency": (i32, [vp, vp, C.POINTER(i32)]),
            "get_observation": (i32, [vp, C.POINTER(TrsObsView)]),
            "fetch_observation": (i32, [vp] + [vp] * 8),
        }
        jpeg = {
            "jpeg_header_bytes": (i32, [vp, i32]),
            "encode_jpeg": (i32, [vp, vp, i32, i32, vp, i32, vp]),
            "encode_jpeg_host": (i32, [vp, vp, i32, i32, i32, vp, C.c_size_t, vp, vp]),
        }
        jpeg_decode = {
            "decode_jpeg": (i32, [vp, vp, vp, vp, i32, vp, vp]),
            "decode_jpeg_host": (i32, [vp, vp, vp, i32, vp, vp]),
        }
        jpeg_codec = {
            "jpeg_roundtrip": (i32, [vp, vp, i32, i32, vp, C.POINTER(vp)]),
            "jpeg_roundtrip_host": (i32, [vp, vp, i32, i32, vp]),
            "set_camera_codec": (i32, [vp, i32]),
            "get_camera_codec": (i32, [vp, C.POINTER(i32)]),
        }
        expert = {
            "default_expert_config": (None, [C.POINTER(TrsExpertConfig)]),
            "set_expert": (i32, [vp, C.POINTER(TrsExpertConfig), vp, vp]),
            "expert_act": (i32, [vp, vp, vp, vp, i32]),
            "step_expert": (i32, [vp, i32, C.POINTER(TrsExpertCapture), C.POINTER(i32)]),
        }
        loader = {
            "default_loader_config": (None, [C.POINTER(TrsLoaderConfig)]),
            "sample_batch": (i32, [vp, C.POINTER(TrsLoaderConfig), vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
            "loader_order": (i32, [C.POINTER(TrsLoaderConfig), i32, i32, i32, i32, vp]),
        }
        dagger = {
            "default_dagger_config": (None, [C.POINTER(TrsDaggerConfig)]),
            "step_dagger": (i32, [vp, C.POINTER(TrsPilotConfig), C.POINTER(TrsDaggerConfig), i32, C.POINTER(TrsExpertCapture), C.POINTER(i32)]),
            "dagger_stats": (i32, [vp, vp, C.POINTER(vp), i32]),
        }
        augment = {
            "default_augment_config": (None, [C.POINTER(TrsAugmentConfig)]),
            "sample_batch_aug": (i32, [vp, C.POINTER(TrsLoaderConfig), C.POINTER(TrsAugmentConfig), vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
            "loader_augment": (i32, [C.POINTER(TrsLoaderConfig), C.POINTER(TrsAugmentConfig), i32, i32, i32, i32, vp, vp, vp]),
        }
        train = {
            "default_train_config": (None, [C.POINTER(TrsTrainConfig)]),
            "pilot_train_begin": (i32, [vp, C.POINTER(TrsTrainConfig), C.POINTER(C.c_void_p)]),
            "pilot_train_step": (i32, [vp, vp, vp, i32, vp]),
            "pilot_train_get": (i32, [vp, C.POINTER(C.c_void_p), C.POINTER(i32)]),
            "pilot_train_debug": (i32, [vp, i32, vp, C.c_size_t]),
            "pilot_train_end": (i32, [vp]),
            "pilot_train_convs": (i32, [vp, C.c_uint32, C.POINTER(C.c_void_p)]),
            "pilot_train_get_convs": (i32, [vp, C.POINTER(C.c_void_p)]),
            "pilot_train_debug_conv": (i32, [vp, i32, i32, vp, C.c_size_t]),
        }
        dropout = {
            "default_dropout_config": (None, [C.POINTER(TrsDropoutConfig)]),
            "pilot_train_dropout": (i32, [vp, C.POINTER(TrsDropoutConfig)]),
            "train_dropout_keep": (i32, [C.POINTER(TrsDropoutConfig), C.c_int64, i32, i32, C.c_int64, vp]),
        }
        train_side = {
            "pilot_train_begin_ex": (i32, [vp, C.POINTER(TrsTrainConfig), C.POINTER(C.c_void_p), i32]),
            "pilot_train_step_ex": (i32, [vp, vp, vp, vp, i32, vp]),
            "pilot_train_get_ex": (i32, [vp, C.POINTER(C.c_void_p), i32, C.POINTER(i32)]),
            "pilot_train_debug_side": (i32, [vp, i32, vp, C.c_size_t]),
        }
        hooks = {"resident_debug_lifetime": (i32, [vp, i32]), "resident_debug_abort": (i32, [vp])}
        for name, (res, args) in sigs.items():
            fn = getattr(cdll, prefix + name)
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)
        self.has_pilot = hasattr(cdll, prefix + "pilot_load")
        if self.has_pilot:
            for name, (res, args) in pilot.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_lens = hasattr(cdll, prefix + "set_camera")
        if self.has_lens:
            for name, (res, args) in lens.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_lighting = hasattr(cdll, prefix + "set_lighting")
        if self.has_lighting:
            for name, (res, args) in light.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_latency = hasattr(cdll, prefix + "set_latency")
        if self.has_latency:
            for name, (res, args) in latency.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_jpeg = hasattr(cdll, prefix + "encode_jpeg")
        if self.has_jpeg:
            for name, (res, args) in jpeg.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_jpeg_decode = hasattr(cdll, prefix + "decode_jpeg")
        if self.has_jpeg_decode:
            for name, (res, args) in jpeg_decode.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_jpeg_codec = hasattr(cdll, prefix + "jpeg_roundtrip")
        if self.has_jpeg_codec:
            for name, (res, args) in jpeg_codec.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_expert = hasattr(cdll, prefix + "set_expert")
        if self.has_expert:
            for name, (res, args) in expert.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_loader = hasattr(cdll, prefix + "sample_batch")
        if self.has_loader:
            for name, (res, args) in loader.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_dagger = hasattr(cdll, prefix + "step_dagger")
        if self.has_dagger:
            for name, (res, args) in dagger.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_augment = hasattr(cdll, prefix + "sample_batch_aug")
        if self.has_augment:
            for name, (res, args) in augment.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_train = hasattr(cdll, prefix + "pilot_train_step")
        if self.has_train:
            for name, (res, args) in train.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_dropout = hasattr(cdll, prefix + "pilot_train_dropout")
        if self.has_dropout:
            for name, (res, args) in dropout.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_train_side = hasattr(cdll, prefix + "pilot_train_step_ex")
        if self.has_train_side:
            for name, (res, args) in train_side.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.has_test_hooks = hasattr(cdll, prefix + "resident_debug_lifetime")
        if self.has_test_hooks:
            for name, (res, args) in hooks.items():
                fn = getattr(cdll, prefix + name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)

    def check(self, rc, what):
        if rc != 0:
            msg = self.last_error()
            raise RuntimeError(f"{self.prefix}{what} failed ({rc}): {msg.decode() if msg else ''}")


def _share_torch_hip_runtime():
    """PyTorch-ROCm ships its own ``libamdhip64``; two HIP runtimes in one process do not both see the GPU
    (``RuntimeError: No HIP GPUs are available`` in whichever loads second).  When torch is installed but not
    imported yet, bind ITS runtime first so that ``libtrsim.so`` and a later ``import torch`` share it; with torch
    already imported (or absent) the loader does the right thing by itself."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    lib = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(lib):
        try:
            C.CDLL(lib, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_hip_library(path=None):
    """Open ``csrc/libtrsim.so`` (built by ``__graft_entry__.build()``); no fallback of any kind."""
    _share_torch_hip_runtime()
    path = path or os.environ.get("TRS_HIP_LIB") or HIP_LIB_PATH      # TRS_HIP_LIB: A/B another HIP build of the same ABI
    if not os.path.exists(path):
        raise RuntimeError(
            f"HIP extension not built: {path} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The product has no CPU fallback.")
    return Api(C.CDLL(path, mode=C.RTLD_LOCAL), "trs_")
