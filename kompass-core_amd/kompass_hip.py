"""ctypes binding of libkompass_hip.so (C ABI: include/kompass_hip.h).

Thin, typed access to the HIP hot path for Python callers (tests, bench.py and
the kompass_core-style wrappers).  There is no CPU fallback: loading fails
loudly when the library has not been built, and every compute call raises
`KompassHipError` when no HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
# KOMPASS_HIP_LIB: another build of the same library (same-box A/B of two builds, tools/ab_libs.sh)
LIB_PATH = Path(os.environ["KOMPASS_HIP_LIB"]) if os.environ.get("KOMPASS_HIP_LIB") else _HERE / "lib" / "libkompass_hip.so"

ACKERMANN, DIFFERENTIAL_DRIVE, OMNI = 0, 1, 2
CYLINDER, BOX, SPHERE = 0, 1, 2
UNEXPLORED, EMPTY, OCCUPIED = -1, 0, 100

KC_OK = 0
_ERR_TO_EXC = {-1: ValueError, -2: IndexError, -3: RuntimeError, -4: NotImplementedError, -5: RuntimeError}


class KompassHipError(RuntimeError):
    pass


class State(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double), ("speed", C.c_double)]


class Limits(C.Structure):
    _fields_ = [
        ("vx_max", C.c_double), ("vx_acc", C.c_double), ("vx_dec", C.c_double),
        ("vy_max", C.c_double), ("vy_acc", C.c_double), ("vy_dec", C.c_double),
        ("omega_max_angle", C.c_double), ("omega_max", C.c_double),
        ("omega_acc", C.c_double), ("omega_dec", C.c_double),
    ]


class Weights(C.Structure):
    _fields_ = [
        ("reference_path_distance_weight", C.c_double),
        ("goal_distance_weight", C.c_double),
        ("obstacles_distance_weight", C.c_double),
        ("smoothness_weight", C.c_double),
        ("jerk_weight", C.c_double),
    ]


class DwaParams(C.Structure):
    _fields_ = [
        ("shape", C.c_int), ("dims", C.c_float * 3), ("ndims", C.c_int),
        ("sensor_pos", C.c_float * 3), ("sensor_rot_xyzw", C.c_float * 4),
        ("octree_res", C.c_double), ("time_step", C.c_double),
        ("max_samples", C.c_size_t), ("max_points", C.c_size_t),
        ("max_segment", C.c_size_t), ("max_obstacles", C.c_size_t),
        ("acc_limits", C.c_float * 3), ("device", C.c_int),
    ]


class StepInputs(C.Structure):
    """kc_step_inputs: one reference controller cycle (kc_dwa_find_best_path)."""
    _fields_ = [
        ("ctr_type", C.c_int), ("limits", C.c_void_p), ("cur_vx", C.c_double), ("cur_vy", C.c_double),
        ("cur_omega", C.c_double), ("max_linear_samples", C.c_int), ("max_angular_samples", C.c_int),
        ("points_xyz", C.c_void_p), ("n_points", C.c_size_t), ("scan_ranges", C.c_void_p), ("scan_angles", C.c_void_p),
        ("n_beams", C.c_size_t), ("max_sensor_range", C.c_float),
        ("seg_xyz", C.c_void_p), ("seg_x", C.c_void_p), ("seg_y", C.c_void_p), ("seg_z", C.c_void_p),
        ("acc_at_seg", C.c_void_p), ("seg_size", C.c_size_t), ("ref_path_length", C.c_float),
        ("num_points", C.c_size_t),
    ]


class Result(C.Structure):
    _fields_ = [
        ("found", C.c_int), ("cost", C.c_float), ("index", C.c_int64),
        ("raw_index", C.c_int64), ("n_admissible", C.c_int64), ("n_samples", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DvzZone(C.Structure):
    """kc_dvz_zone: the zone of DeformableVirtualZone (algorithms/dvz.py)."""
    _fields_ = [("major_radius", C.c_double), ("minor_radius", C.c_double),
                ("center_shift_x", C.c_double), ("center_shift_y", C.c_double), ("ori_shift", C.c_double)]


class WorldMapPose(C.Structure):
    """kc_worldmap_pose: the local grid's frame in the map, 16 fraction bits."""
    _fields_ = [("cq", C.c_int32), ("sq", C.c_int32), ("tx", C.c_int64), ("ty", C.c_int64)]


class WorldMapResult(C.Structure):
    """kc_worldmap_result: what an update did to the cls plane."""
    _fields_ = [("changed", C.c_uint32), ("i_min", C.c_int32), ("j_min", C.c_int32), ("i_max", C.c_int32),
                ("j_max", C.c_int32)]

    def as_tuple(self):
        """(changed, (i_min, j_min, i_max, j_max)); the box is all -1 when nothing changed."""
        return int(self.changed), (int(self.i_min), int(self.j_min), int(self.i_max), int(self.j_max))


class WorldMapCluster(C.Structure):
    """kc_worldmap_cluster: rule 68's record of a kept cluster, 64 bytes."""
    _fields_ = [("k_first", C.c_int32), ("k_last", C.c_int32), ("n", C.c_int32), ("reserved", C.c_int32),
                ("sx", C.c_int64), ("sy", C.c_int64), ("min_x", C.c_int64), ("max_x", C.c_int64), ("min_y", C.c_int64),
                ("max_y", C.c_int64)]

    def as_tuple(self):
        """(k_first, k_last, n, sx, sy, min_x, max_x, min_y, max_y)"""
        return (int(self.k_first), int(self.k_last), int(self.n), int(self.sx), int(self.sy), int(self.min_x), int(self.max_x),
                int(self.min_y), int(self.max_y))


class WorldMapMoversRecord(C.Structure):
    """kc_worldmap_movers_record: rule 69's counts."""
    _fields_ = [("n_dynamic", C.c_uint32), ("n_runs", C.c_uint32), ("n_kept", C.c_uint32), ("n_returned", C.c_uint32)]

    def as_tuple(self):
        """(n_dynamic, n_runs, n_kept, n_returned)"""
        return int(self.n_dynamic), int(self.n_runs), int(self.n_kept), int(self.n_returned)


class WorldMapRotation(C.Structure):
    """kc_worldmap_rotation: one rotation of a match's window, 16 fraction bits."""
    _fields_ = [("cq", C.c_int32), ("sq", C.c_int32)]


class WorldMapMatchResult(C.Structure):
    """kc_worldmap_match_result: the winner of a match (DESIGN.md 4.11 rule 15)."""
    _fields_ = [("k", C.c_int32), ("u", C.c_int32), ("v", C.c_int32), ("score", C.c_uint32), ("score_guess", C.c_uint32),
                ("n_points", C.c_uint32), ("pose", WorldMapPose)]

    def as_dict(self):
        """k, u, v, score, score_guess, points, and pose: the corrected (cq, sq, tx, ty)."""
        p = self.pose
        return dict(k=int(self.k), u=int(self.u), v=int(self.v), score=int(self.score), score_guess=int(self.score_guess),
                    points=int(self.n_points), pose=(int(p.cq), int(p.sq), int(p.tx), int(p.ty)))


class MclRecord(C.Structure):
    """kc_mcl_record: the exact sums of one localiser step (DESIGN.md 4.11 rule 37)."""
    _fields_ = [("w1", C.c_uint64), ("w2", C.c_uint64), ("sx_lo", C.c_uint64), ("sx_hi", C.c_int64),
                ("sy_lo", C.c_uint64), ("sy_hi", C.c_int64), ("sc", C.c_int64), ("ss", C.c_int64),
                ("best_tx", C.c_int64), ("best_ty", C.c_int64), ("best_h", C.c_uint32), ("amin", C.c_uint32),
                ("best", C.c_uint32), ("step", C.c_uint32)]

    @property
    def sx(self):
        """SX as a Python int: (hi << 64) + lo."""
        return (int(self.sx_hi) << 64) + int(self.sx_lo)

    @property
    def sy(self):
        return (int(self.sy_hi) << 64) + int(self.sy_lo)

    def as_tuple(self):
        """(w1, w2, sx, sy, sc, ss, amin, best, best_tx, best_ty, best_h, step)"""
        return (int(self.w1), int(self.w2), self.sx, self.sy, int(self.sc), int(self.ss), int(self.amin), int(self.best),
                int(self.best_tx), int(self.best_ty), int(self.best_h), int(self.step))


class MclFit(C.Structure):
    """kc_mcl_fit: the absolute penalties of one localiser step (DESIGN.md 4.11 rule 59)."""
    _fields_ = [("cost_sum", C.c_uint64), ("cost_min", C.c_uint32), ("cost_best", C.c_uint32), ("step", C.c_uint32)]

    def as_tuple(self):
        """(cost_sum, cost_min, cost_best, step)"""
        return int(self.cost_sum), int(self.cost_min), int(self.cost_best), int(self.step)


class MppiRecord(C.Structure):
    """kc_mppi_record: one controller step (DESIGN.md 4.12 rules 11 and 17).  n_hit_moving: the samples among n_hit that a
    moving obstacle ended, 0 with none set."""
    _fields_ = [("den", C.c_uint64), ("s_min", C.c_uint32), ("k_best", C.c_uint32), ("s_0", C.c_uint32),
                ("n_hit", C.c_uint32), ("step", C.c_uint32), ("n_hit_moving", C.c_uint32)]

    def as_tuple(self):
        """(s_min, k_best, s_0, den, n_hit, step)"""
        return int(self.s_min), int(self.k_best), int(self.s_0), int(self.den), int(self.n_hit), int(self.step)


class MclRecovery(C.Structure):
    """kc_mcl_recovery: rule 61's two averages."""
    _fields_ = [("slow", C.c_int64), ("fast", C.c_int64), ("primed", C.c_int32)]


_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p
_sz = C.c_size_t

# every symbol include/kompass_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "kc_last_error": (C.c_char_p, []),
    "kc_abi_version": (C.c_int, []),
    "kc_device_count": (C.c_int, []),
    "kc_dwa_create": (C.c_int, [C.POINTER(DwaParams), C.POINTER(_vp)]),
    "kc_dwa_destroy": (None, [_vp]),
    "kc_dwa_set_stream": (C.c_int, [_vp, _vp]),
    "kc_dwa_set_resolution": (C.c_int, [_vp, C.c_double]),
    "kc_dwa_set_weights": (C.c_int, [_vp, C.POINTER(Weights)]),
    "kc_dwa_set_option": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "kc_dwa_get_option": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    "kc_set_host_threads": (C.c_int, [C.c_int]),
    "kc_trig_selfcheck": (C.c_int, [C.POINTER(C.c_int64)]),
    "kc_trig_table": (C.c_int, [C.c_double, _dp, _sz, _sz, C.c_double, _dp]),
    "kc_dwa_sample_window": (C.c_int, [_vp, C.c_int, C.POINTER(Limits), C.c_double, C.c_double, C.c_double,
                                       C.c_int, C.c_int, C.POINTER(_sz), _dp, _dp, _dp, _sz]),
    "kc_dwa_set_samples": (C.c_int, [_vp, _sz, _dp, _dp, _dp]),
    "kc_dwa_set_shard": (C.c_int, [_vp, _sz, _sz]),
    "kc_dwa_set_shard_rule": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "kc_shard_plan": (C.c_int, [_ip, _sz, C.c_int, C.c_int, _ip]),
    "kc_shard_merge": (C.c_int, [C.POINTER(C.c_int64), _sz, C.c_int, C.c_int, _ip, _sz, C.POINTER(Result)]),
    "kc_dwa_owns_sample": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int)]),
    "kc_dwa_set_scan": (C.c_int, [_vp, C.POINTER(State), _dp, _dp, _sz, C.c_float]),
    "kc_dwa_set_points": (C.c_int, [_vp, C.POINTER(State), _fp, _sz, C.c_float]),
    "kc_dwa_set_points_sensor_frame": (C.c_int, [_vp, C.POINTER(State), _fp, _sz, C.c_float]),
    "kc_dwa_set_path": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _sz, C.c_float]),
    "kc_dwa_set_tracked_window": (C.c_int, [_vp, _sz, _sz]),
    "kc_dwa_set_grid_device": (C.c_int, [_vp, C.POINTER(State), _vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                         C.c_float]),
    "kc_dwa_set_grid_from_mapper": (C.c_int, [_vp, C.POINTER(State), _vp, C.c_float]),
    "kc_dwa_set_worldmap": (C.c_int, [_vp, C.POINTER(State), _vp, C.c_float]),
    "kc_dwa_set_tracked_segment": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _sz, C.c_float]),
    "kc_dwa_set_tracked_segment_xyz": (C.c_int, [_vp, _fp, _fp, _sz, C.c_float]),
    "kc_dwa_rollout": (C.c_int, [_vp, C.POINTER(State), _sz]),
    "kc_dwa_check_poses": (C.c_int, [_vp, _dp, _dp, _dp, _sz, C.POINTER(C.c_uint8)]),
    "kc_dwa_first_clear_command": (C.c_int, [_vp, C.POINTER(State), _dp, _dp, _dp, _sz, C.c_int, C.c_double,
                                             C.POINTER(C.c_int64)]),
    "kc_dwa_evaluate": (C.c_int, [_vp]),
    "kc_dwa_fetch_result": (C.c_int, [_vp, C.POINTER(Result)]),
    "kc_dwa_cycle": (C.c_int, [_vp, C.POINTER(State), _sz, C.POINTER(Result)]),
    "kc_dwa_find_best_path": (C.c_int, [_vp, C.POINTER(State), C.POINTER(StepInputs), C.POINTER(Result)]),
    "kc_dwa_get_best": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _fp]),
    "kc_dwa_get_sample_velocity": (C.c_int, [_vp, C.c_int64, _dp, _dp, _dp]),
    "kc_dwa_get_samples": (C.c_int, [_vp, _fp, _fp, _ip, _fp, _sz, C.POINTER(_sz)]),
    "kc_dwa_get_freeze_steps": (C.c_int, [_vp, _ip, _sz, C.POINTER(_sz)]),
    "kc_cost_evaluate": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _fp, _sz, _sz, _fp, C.POINTER(Result)]),
    "kc_cost_upload": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _fp, _sz, _sz]),
    "kc_cost_evaluate_resident": (C.c_int, [_vp, _fp, C.POINTER(Result)]),
    "kc_dwa_result_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "kc_dwa_publish_result": (C.c_int, [_vp]),
    "kc_dwa_count_admissible_before": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64)]),
    "kc_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "kc_comm_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.POINTER(_vp)]),
    "kc_comm_create_shm": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(_vp)]),
    "kc_comm_transport": (C.c_int, [_vp]),
    "kc_comm_query": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kc_comm_destroy": (None, [_vp]),
    "kc_comm_rank": (C.c_int, [_vp]),
    "kc_comm_world": (C.c_int, [_vp]),
    "kc_dwa_allreduce_best": (C.c_int, [_vp, _vp]),
    "kc_dwa_cycle_sharded": (C.c_int, [_vp, _vp, C.POINTER(State), _sz, C.POINTER(Result)]),
    "kc_dwa_exchange_best": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_int64, C.POINTER(Result)]),
    "kc_dwa_global_index": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "kc_key_cost": (C.c_float, [C.c_int64]),
    "kc_key_index": (C.c_int64, [C.c_int64]),
    "kc_key_pack": (C.c_int64, [C.c_float, C.c_int64]),
    "kc_dwa_timing_enable": (C.c_int, [_vp, C.c_int]),
    "kc_dwa_timing_get": (C.c_int, [_vp, C.POINTER(C.c_char_p), _fp, _sz, C.POINTER(_sz)]),
    "kc_mapper_create": (C.c_int, [C.c_int, C.c_int, C.c_float, _fp, C.c_float, _sz, C.c_int, C.POINTER(_vp)]),
    "kc_mapper_destroy": (None, [_vp]),
    "kc_mapper_set_stream": (C.c_int, [_vp, _vp]),
    "kc_mapper_scan_to_grid": (C.c_int, [_vp, _dp, _dp, _sz, _ip]),
    "kc_mapper_scan_to_grid_device": (C.c_int, [_vp, _dp, _dp, _sz]),
    "kc_mapper_grid_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "kc_mapper_enable_bayes": (C.c_int, [_vp, C.c_void_p]),
    "kc_mapper_scan_to_grid_bayes": (C.c_int, [_vp, _dp, _dp, _sz, _ip, _fp]),
    "kc_mapper_scan_to_grid_bayes_device": (C.c_int, [_vp, _dp, _dp, _sz]),
    "kc_mapper_prob_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "kc_mapper_warp_previous": (C.c_int, [_vp, _fp, C.c_double]),
    "kc_mapper_get_previous_prob": (C.c_int, [_vp, _fp]),
    "kc_mapper_set_previous_prob": (C.c_int, [_vp, _fp]),
    "kc_mapper_sync": (C.c_int, [_vp]),
    "kc_mapper_timing_enable": (C.c_int, [_vp, C.c_int]),
    "kc_mapper_timing_get": (C.c_int, [_vp, C.POINTER(C.c_char_p), _fp, _sz, C.POINTER(_sz)]),
    "kc_zone_create": (C.c_int, [C.c_int, _fp, C.c_int, _fp, _fp, C.c_float, C.c_float, C.c_float, _dp, _sz,
                                 C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(_vp)]),
    "kc_zone_destroy": (None, [_vp]),
    "kc_zone_check": (C.c_int, [_vp, _dp, _sz, C.c_int, C.POINTER(C.c_float)]),
    "kc_zone_check_cloud": (C.c_int, [_vp, C.c_void_p, _sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "kc_zone_indices": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64), _sz, C.POINTER(_sz)]),
    "kc_cloud_create": (C.c_int, [_sz, _sz, C.c_int, C.POINTER(_vp)]),
    "kc_cloud_destroy": (None, [_vp]),
    "kc_cloud_to_laserscan": (C.c_int, [_vp, C.c_void_p, _sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                        C.c_double, C.c_int, _dp, _dp, _sz, C.POINTER(_sz)]),
    "kc_cloud_to_laserscan_typed": (C.c_int, [_vp, C.c_void_p, _sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                              C.c_int, _dp, _dp, _sz, C.POINTER(_sz)]),
    "kc_zone_check_cloud_typed": (C.c_int, [_vp, C.c_void_p, _sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_int, _fp]),
    "kc_cloud_grid_extent": (C.c_int, [_vp, C.c_void_p, _sz, C.c_int, C.c_int, _sz, C.c_int, C.c_int, C.c_int,
                                       C.c_float, _fp, _ip, _ip]),
    "kc_cloud_grid_fill": (C.c_int, [_vp, C.c_float, C.c_float, C.c_void_p, _sz]),
    "kc_cloud_grid_device": (C.c_int, [_vp, C.c_float, C.c_float, C.POINTER(_vp)]),
    "kc_cloud_after_stream": (C.c_int, [_vp, C.c_void_p]),
    "kc_cloud_last_rebinned": (C.c_int, [_vp, C.POINTER(_sz)]),
    "kc_cloud_timing_enable": (C.c_int, [_vp, C.c_int]),
    "kc_cloud_timing_get": (C.c_int, [_vp, C.POINTER(C.c_char_p), _fp, _sz, C.POINTER(_sz)]),
    "kc_depth_create": (C.c_int, [_fp, _fp, _fp, _fp, _fp, C.c_float, C.c_int, C.POINTER(_vp)]),
    "kc_depth_destroy": (None, [_vp]),
    "kc_depth_boxes": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _ip, _sz, _dp,
                                 _fp, _ip, _sz, C.POINTER(_sz)]),
    "kc_depth_box_stats": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _ip, _sz,
                                     C.POINTER(C.c_int64), _fp]),
    "kc_depth_after_stream": (C.c_int, [_vp, C.c_void_p]),
    "kc_depth_last_upload": (C.c_int, [_vp, C.POINTER(_sz)]),
    "kc_depth_timing_enable": (C.c_int, [_vp, C.c_int]),
    "kc_depth_timing_get": (C.c_int, [_vp, C.POINTER(C.c_char_p), _fp, _sz, C.POINTER(_sz)]),
    "kc_dvz_create": (C.c_int, [C.c_int, _sz, C.POINTER(_vp)]),
    "kc_dvz_destroy": (None, [_vp]),
    "kc_dvz_deform": (C.c_int, [_vp, C.POINTER(DvzZone), _dp, _dp, _sz, _dp, _dp]),
    "kc_planner_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "kc_planner_destroy": (None, [_vp]),
    "kc_planner_set_grid_host": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kc_planner_set_grid_device": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kc_planner_after_stream": (C.c_int, [_vp, C.c_void_p]),
    "kc_planner_solve": (C.c_int, [_vp, _ip, _ip, C.c_uint32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_int)]),
    "kc_planner_get_field": (C.c_int, [_vp, C.c_void_p, C.c_void_p, _sz]),
    "kc_planner_get_path": (C.c_int, [_vp, C.c_void_p, _sz, C.POINTER(_sz)]),
    "kc_planner_set_clearance_cost": (C.c_int, [_vp, C.c_uint32, C.c_void_p, _sz]),
    "kc_planner_get_clearance": (C.c_int, [_vp, C.c_void_p, C.c_void_p, _sz]),
    "kc_planner_path_clearance": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "kc_planner_shortcut": (C.c_int, [_vp, C.c_int, C.POINTER(_sz), C.POINTER(C.c_uint32)]),
    "kc_planner_get_shortcut": (C.c_int, [_vp, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz)]),
    "kc_planner_set_oriented": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "kc_planner_solve_oriented": (C.c_int, [_vp, _ip, C.c_int, _ip, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_int)]),
    "kc_planner_get_oriented_field": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_void_p, _sz]),
    "kc_planner_get_oriented_path": (C.c_int, [_vp, C.c_void_p, _sz, C.POINTER(_sz)]),
    "kc_planner_set_car": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]),
    "kc_planner_solve_car": (C.c_int, [_vp, _ip, C.c_int, _ip, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "kc_planner_get_car_field": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_void_p, _sz]),
    "kc_planner_get_car_path": (C.c_int, [_vp, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz)]),
    "kc_planner_car_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "kc_planner_replan": (C.c_int, [_vp, _ip, _ip, C.c_uint32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_int)]),
    "kc_planner_replan_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]),
    "kc_planner_explore": (C.c_int, [_vp, _ip, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                     C.POINTER(_sz), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kc_planner_get_frontiers": (C.c_int, [_vp, C.c_void_p, _sz, C.POINTER(_sz)]),
    "kc_planner_get_frontier_path": (C.c_int, [_vp, _sz, C.c_void_p, _sz, C.POINTER(_sz)]),
    "kc_planner_get_frontier_labels": (C.c_int, [_vp, C.c_void_p, _sz]),
    "kc_planner_explore_info": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "kc_worldmap_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, C.c_double, C.POINTER(_vp)]),
    "kc_worldmap_destroy": (None, [_vp]),
    "kc_worldmap_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, _dp, _dp]),
    "kc_worldmap_check_model": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kc_worldmap_set_model": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kc_worldmap_quantise_pose": (C.c_int, [C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                            C.POINTER(WorldMapPose)]),
    "kc_worldmap_check_grid": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "kc_worldmap_update_device": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                            C.POINTER(WorldMapPose), C.POINTER(WorldMapResult)]),
    "kc_worldmap_update_host": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.POINTER(WorldMapPose), C.POINTER(WorldMapResult)]),
    "kc_worldmap_update_from_mapper": (C.c_int, [_vp, _vp, C.POINTER(WorldMapPose), C.POINTER(WorldMapResult)]),
    "kc_worldmap_set_prior_host": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kc_worldmap_set_prior_device": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kc_worldmap_after_stream": (C.c_int, [_vp, C.c_void_p]),
    "kc_worldmap_clear": (C.c_int, [_vp]),
    "kc_worldmap_grid_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "kc_worldmap_get": (C.c_int, [_vp, C.c_void_p, C.c_void_p, _sz]),
    "kc_worldmap_window": (C.c_int, [C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kc_worldmap_points": (C.c_int, [_vp, C.c_double, C.c_double, C.c_float, C.c_void_p, _sz, C.POINTER(_sz),
                                     C.POINTER(C.c_int32)]),
    "kc_worldmap_scan_table": (C.c_int, [_dp, _sz, _ip]),
    "kc_worldmap_scan_check": (C.c_int, [C.c_float, _sz, _sz, C.c_float, C.c_uint, _ip]),
    "kc_worldmap_scan": (C.c_int, [_vp, C.POINTER(WorldMapPose), _sz, _dp, _sz, C.c_float, C.c_uint, _dp, _ip]),
    "kc_dvz_deform_worldmap": (C.c_int, [_vp, C.POINTER(DvzZone), _vp, C.POINTER(WorldMapPose), _dp, _sz, C.c_float,
                                         C.c_uint, _dp, _dp, _dp, _dp]),
    "kc_zone_check_worldmap": (C.c_int, [_vp, _vp, C.POINTER(WorldMapPose), C.c_uint, _dp, C.c_int,
                                         C.POINTER(C.c_float)]),
    "kc_worldmap_match_check_window": (C.c_int, [C.c_int, C.c_double, C.c_int]),
    "kc_worldmap_match_check_grid": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "kc_worldmap_match_rotations": (C.c_int, [C.c_double, C.c_int, C.c_double, C.POINTER(WorldMapRotation), _sz]),
    "kc_worldmap_match_device": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.POINTER(WorldMapPose), C.POINTER(WorldMapRotation), C.c_int, C.c_int,
                                           C.POINTER(WorldMapMatchResult)]),
    "kc_worldmap_match_host": (C.c_int, [_vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.POINTER(WorldMapPose), C.POINTER(WorldMapRotation), C.c_int, C.c_int,
                                         C.POINTER(WorldMapMatchResult)]),
    "kc_worldmap_match_from_mapper": (C.c_int, [_vp, _vp, C.POINTER(WorldMapPose), C.POINTER(WorldMapRotation), C.c_int,
                                                C.c_int, C.POINTER(WorldMapMatchResult)]),
    "kc_worldmap_match_scores": (C.c_int, [_vp, C.c_void_p, _sz]),
    "kc_worldmap_match_set_timing": (C.c_int, [_vp, C.c_int]),
    "kc_worldmap_match_times": (C.c_int, [_vp, _fp]),
    "kc_mcl_check": (C.c_int, [C.c_float, _sz, _sz, C.c_float, C.c_void_p, _sz, C.c_int, C.c_void_p, _sz, C.c_int, C.c_uint,
                               _ip, C.POINTER(C.c_int64)]),
    "kc_mcl_heading": (C.c_int, [C.c_uint32, _ip, _ip]),
    "kc_mcl_create": (C.c_int, [_vp, _sz, _dp, _sz, C.c_float, C.c_uint64, C.POINTER(_vp)]),
    "kc_mcl_destroy": (None, [_vp]),
    "kc_mcl_info": (C.c_int, [_vp, C.POINTER(_sz), C.POINTER(_sz), _ip, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)]),
    "kc_mcl_set_model": (C.c_int, [_vp, C.c_void_p, _sz, C.c_int, C.c_void_p, _sz, C.c_int]),
    "kc_mcl_init_pose": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_uint32, C.c_int32, C.c_int32]),
    "kc_mcl_init_global": (C.c_int, [_vp, C.POINTER(_sz)]),
    "kc_mcl_step": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip, C.c_uint,
                              C.POINTER(MclRecord)]),
    "kc_mcl_resample": (C.c_int, [_vp]),
    "kc_mcl_particles": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _sz]),
    "kc_mcl_particles_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "kc_mcl_set_timing": (C.c_int, [_vp, C.c_int]),
    "kc_mcl_times": (C.c_int, [_vp, _fp]),
    "kc_worldmap_set_distance": (C.c_int, [_vp, C.c_int, C.c_uint]),
    "kc_worldmap_distance_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kc_worldmap_distance_refresh": (C.c_int, [_vp]),
    "kc_worldmap_get_distance": (C.c_int, [_vp, C.c_void_p, _sz]),
    "kc_worldmap_distance_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "kc_mcl_field_check": (C.c_int, [C.c_float, _sz, _sz, C.c_float, C.c_void_p, _sz, C.c_int, C.c_void_p, _sz, C.c_int, C.c_uint,
                                     _ip, C.POINTER(C.c_int64)]),
    "kc_mcl_set_field_model": (C.c_int, [_vp, C.c_void_p, _sz, C.c_uint16, C.c_void_p, _sz, C.c_int]),
    "kc_mcl_model_kind": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "kc_worldmap_shift": (C.c_int, [_vp, C.c_int, C.c_int]),
    "kc_worldmap_check_shift": (C.c_int, [C.c_int32, C.c_int32, C.c_int, C.c_int]),
    "kc_worldmap_offset": (C.c_int, [_vp, _ip, _ip]),
    "kc_worldmap_recentre_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip]),
    "kc_worldmap_recentre": (C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.c_int, _ip, _ip]),
    "kc_worldmap_integrate_check": (C.c_int, [C.c_float, _sz, C.c_float, C.c_uint, C.c_void_p, _ip, C.POINTER(C.c_int64)]),
    "kc_worldmap_quantise_ranges": (C.c_int, [C.c_float, _dp, _sz, C.c_float, C.c_float, _ip]),
    "kc_worldmap_integrate": (C.c_int, [_vp, C.POINTER(WorldMapPose), _dp, _sz, _ip, C.c_float, C.c_uint,
                                        C.POINTER(WorldMapResult)]),
    "kc_worldmap_integrate_marks": (C.c_int, [_vp, C.POINTER(WorldMapPose), _dp, _sz, _ip, C.c_float, C.c_uint, C.c_void_p, _sz]),
    "kc_worldmap_integrate_set_precheck": (C.c_int, [_vp, C.c_int]),
    "kc_worldmap_integrate_set_timing": (C.c_int, [_vp, C.c_int]),
    "kc_worldmap_integrate_times": (C.c_int, [_vp, _fp]),
    "kc_worldmap_movers_check": (C.c_int, [C.c_float, _sz, C.c_float, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                           C.POINTER(C.c_int64)]),
    "kc_worldmap_movers": (C.c_int, [_vp, C.POINTER(WorldMapPose), _dp, _sz, _ip, C.c_float, C.c_uint32, C.c_uint32, C.c_uint64,
                                     C.c_uint32, C.c_void_p, C.POINTER(WorldMapCluster), _sz,
                                     C.POINTER(WorldMapMoversRecord)]),
    "kc_worldmap_movers_set_timing": (C.c_int, [_vp, C.c_int]),
    "kc_worldmap_movers_times": (C.c_int, [_vp, _fp]),
    "kc_mcl_last_fit": (C.c_int, [_vp, C.POINTER(MclFit)]),
    "kc_mcl_recovery_update": (C.c_int, [C.c_uint64, _sz, _sz, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(MclRecovery),
                                         C.POINTER(C.c_int64), C.POINTER(_sz)]),
    "kc_mcl_resample_inject": (C.c_int, [_vp, _sz]),
    "kc_mcl_inject_times": (C.c_int, [_vp, _fp]),
    "kc_mppi_check": (C.c_int, [_sz, _sz, _sz, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, _sz, C.c_uint32, C.c_uint32,
                                C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, _sz, C.c_int]),
    "kc_mppi_create": (C.c_int, [_vp, _sz, _sz, C.c_uint64, C.POINTER(_vp)]),
    "kc_mppi_destroy": (None, [_vp]),
    "kc_mppi_set_model": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "kc_mppi_set_costs": (C.c_int, [_vp, C.c_uint32, C.c_void_p, _sz, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                    C.c_void_p, _sz, C.c_int]),
    "kc_mppi_set_path": (C.c_int, [_vp, C.c_void_p, C.c_void_p, _sz]),
    "kc_mppi_check_movers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _sz,
                                       C.c_uint32]),
    "kc_mppi_set_movers": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _sz,
                                     C.c_uint32]),
    "kc_mppi_check_field": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "kc_mppi_set_field": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "kc_mppi_last_field": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "kc_mppi_check_rates": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kc_mppi_set_rates": (C.c_int, [_vp, C.c_void_p]),
    "kc_mppi_set_velocity": (C.c_int, [_vp, C.c_void_p]),
    "kc_mppi_apply_rates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_void_p]),
    "kc_mppi_check_footprint": (C.c_int, [C.c_void_p, _sz]),
    "kc_mppi_set_footprint": (C.c_int, [_vp, C.c_void_p, _sz]),
    "kc_planner_field_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "kc_mppi_step": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(MppiRecord)]),
    "kc_mppi_costs": (C.c_int, [_vp, C.c_void_p, _sz]),
    "kc_mppi_set_team": (C.c_int, [_vp, C.c_int]),
    "kc_mppi_set_timing": (C.c_int, [_vp, C.c_int]),
    "kc_mppi_times": (C.c_int, [_vp, _fp]),
}

_lib = None

# The four calls of a controller cycle with fresh inputs (window, points, segment, cycle) sit on the critical
# path in front of the cycle kernel's launch: a second prototype of each takes plain ADDRESSES (c_void_p from an
# int: no ctypes pointer objects per call), the wrappers below reuse one State / Result per context and hand
# float32 C-contiguous arrays over where they lie.
_fast = {}


def _fast_protos():
    vp, i, d, f, z = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_size_t
    return {
        "kc_dwa_set_points": (vp, vp, vp, z, f),
        "kc_dwa_set_tracked_segment": (vp, vp, vp, vp, vp, z, f),
        "kc_dwa_set_tracked_segment_xyz": (vp, vp, vp, z, f),
        "kc_dwa_cycle": (vp, vp, z, vp),
        "kc_dwa_find_best_path": (vp, vp, vp, vp),
        "kc_dwa_sample_window": (vp, i, vp, d, d, d, i, i, vp, vp, vp, vp, z),
    }


def _missing(name, path):
    def stub(*_args):
        raise KompassHipError(f"{name} is not exported by {path} (loaded with tolerant=True)")
    return stub


def load(path=None, tolerant=False):
    """Load the library at `path` (default: LIB_PATH), give every entry of SIGNATURES its prototype, bind `_fast`
    and make it the library `lib()` returns.  A symbol the library does not export fails the load -- or, with
    tolerant=True (an OLDER build in a same-box A/B, tools/ab_libs.sh), is bound to a stub, in the library object
    and in `_fast`, that raises KompassHipError when it is called."""
    global _lib
    path = str(LIB_PATH if path is None else path)  # a file, or a name for the dynamic loader to find
    try:
        L = C.CDLL(path)
    except OSError:
        if os.path.exists(path):
            raise
        raise KompassHipError(
            f"{path} is missing: build it with `make -C {_HERE}` "
            "(or __graft_entry__.build()); there is no CPU fallback") from None
    protos, fast = _fast_protos(), {}
    for name, (res, args) in SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
            if name in protos:
                fast[name] = C.CFUNCTYPE(C.c_int, *protos[name])((name, L))
        elif tolerant:
            setattr(L, name, _missing(name, path))
            if name in protos:
                fast[name] = getattr(L, name)
        else:
            raise KompassHipError(f"{path} does not export {name}: not a build of this version of the library")
    _fast.update(fast)
    _lib = L
    return L


def lib():
    """The loaded libkompass_hip.so (raises if it was not built -- no fallback).  KOMPASS_HIP_LIB selects another
    build (LIB_PATH), KOMPASS_HIP_LIB_OLD=1 loads it tolerantly: both are hooks of tools/ab_libs.sh."""
    if _lib is not None:
        return _lib
    return load(tolerant=os.environ.get("KOMPASS_HIP_LIB_OLD") == "1")


def _addr32(a):
    """(float32 C-contiguous array, its address): `a` itself when it already is one."""
    if not (type(a) is np.ndarray and a.dtype == np.float32 and a.flags.c_contiguous):
        a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.__array_interface__["data"][0]


def _check(rc):
    if rc != KC_OK:
        msg = lib().kc_last_error().decode("utf-8", "replace")
        exc = _ERR_TO_EXC.get(rc, KompassHipError)
        if exc is RuntimeError:
            exc = KompassHipError
        raise exc(f"[kc {rc}] {msg}")


def device_count() -> int:
    return lib().kc_device_count()


def set_host_threads(n: int):
    """Threads of the process-wide host pool behind the roll-out's libm trig table."""
    _check(lib().kc_set_host_threads(int(n)))


def trig_selfcheck() -> int:
    """The restated sincos (csrc/kc_trig_exact.h) against the installed libm on the library's fixed argument
    set (host only); returns the number of arguments compared, raises when any differs."""
    return int(_out(C.c_int64, lib().kc_trig_selfcheck))


def trig_table(yaw0: float, omega, n_steps: int, dt: float):
    """{cos, sin}(yaw_k) of every omega row, formed on the device: [n_steps, n_rows, 2] float64."""
    om = np.ascontiguousarray(omega, dtype=np.float64)
    out = np.empty((int(n_steps), len(om), 2), dtype=np.float64)
    _check(lib().kc_trig_table(float(yaw0), om.ctypes.data_as(_dp), len(om), int(n_steps), float(dt),
                               out.ctypes.data_as(_dp)))
    return out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _pf(a):
    return a.ctypes.data_as(_fp) if a is not None else None


def _pd(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _out(ctype, fn, *args):
    """fn(*args, &v) with v a zeroed `ctype`, checked -> v.value: the calls with one out-parameter, the last."""
    v = ctype()
    _check(fn(*args, C.byref(v)))
    return v.value


def _fill(fn, h, specs):
    """The two calls of a list getter: fn(h, NULL ..., 0, &n) asks for the count, fn(h, arrays ..., n, &n) fills
    one array per entry of `specs` -- (dtype, shape of one element), or None for an output that is not wanted.
    -> the arrays cut to n rows (None where the spec is)."""
    n = _sz(0)
    _check(fn(h, *[None] * len(specs), 0, C.byref(n)))
    k = n.value
    out = [None if s is None else np.zeros((max(k, 1),) + s[1], s[0]) for s in specs]
    if k:
        ptrs = [a if a is None else a.ctypes.data_as(t) for a, t in zip(out, fn.argtypes[1:])]
        _check(fn(h, *ptrs, k, C.byref(n)))
    return [a if a is None else a[:k] for a in out]


class _Owner:
    """Owner of one context of the library: the handle `h`, and the one way it is released.  A subclass names its
    C prefix (`_kc`: kc_dwa_destroy is its destroy function) and opens the handle with `_open`."""
    _kc = None

    def _open(self, create, *args):
        """create(*args, &h), checked."""
        self.h = _vp()
        _check(create(*args, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            getattr(lib(), self._kc + "_destroy")(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _Timed:
    """Per-kernel timing of a context (kc_*_timing_enable / kc_*_timing_get); `_timing_cap` is the most entries
    `timings` asks for."""
    _timing_cap = 16

    def timing_enable(self, on=True):
        _check(getattr(lib(), self._kc + "_timing_enable")(self.h, int(bool(on))))

    def timings(self):
        cap = self._timing_cap
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = _sz(0)
        _check(getattr(lib(), self._kc + "_timing_get")(self.h, names, ms, cap, C.byref(n)))
        return [(names[i].decode(), float(ms[i])) for i in range(n.value)]


class _StreamOrdered:
    def after_stream(self, stream=None):
        """Order the context's next read of a device buffer it is handed after the work queued so far on `stream`
        (a hipStream_t address; None: the legacy default stream)."""
        _check(getattr(lib(), self._kc + "_after_stream")(self.h, stream))


def make_limits(vx=(1.0, 10.0, 10.0), vy=(1.0, 10.0, 10.0), omega=(np.pi, 1.0, 10.0, 10.0)) -> Limits:
    return Limits(vx[0], vx[1], vx[2], vy[0], vy[1], vy[2], omega[0], omega[1], omega[2], omega[3])


def make_weights(path=1.0, goal=1.0, obstacles=1.0, smoothness=1.0, jerk=1.0) -> Weights:
    return Weights(path, goal, obstacles, smoothness, jerk)


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI: call on one rank, send the bytes to every rank."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().kc_comm_unique_id(buf))
    return bytes(buf)


SHARD_BLOCKS, SHARD_ROWS = 0, 1
COMM_RCCL, COMM_SHM = 0, 1


def shard_plan(rows, world: int, mode: int = SHARD_ROWS):
    """kc_shard_plan: owner rank of every sample from its trig row (pure host function)."""
    rows = np.ascontiguousarray(rows, np.int32)
    owner = np.zeros(len(rows), np.int32)
    _check(lib().kc_shard_plan(rows.ctypes.data_as(_ip), len(rows), int(world), int(mode),
                               owner.ctypes.data_as(_ip)))
    return owner


def shard_merge(record, words_per_rank: int, world: int, mode: int, owner, n_total: int) -> Result:
    """kc_shard_merge: the reduced exchange record -> result (pure host function)."""
    rec = np.ascontiguousarray(record, np.int64)
    own = None if owner is None else np.ascontiguousarray(owner, np.int32)
    r = Result()
    _check(lib().kc_shard_merge(rec.ctypes.data_as(C.POINTER(C.c_int64)), int(words_per_rank), int(world), int(mode),
                                None if own is None else own.ctypes.data_as(_ip), int(n_total), C.byref(r)))
    return r


class Comm(_Owner):
    """Owner of one kc_comm: an RCCL communicator inside libkompass_hip.so, or -- shm_name given --
    the shared-memory rehearsal transport for ranks that share a GPU (kc_comm_create_shm)."""
    _kc = "kc_comm"

    def __init__(self, rank: int, world: int, unique_id: bytes = None, device: int = 0, shm_name: str = None):
        if shm_name is not None:
            self._open(lib().kc_comm_create_shm, int(rank), int(world), shm_name.encode(), int(device))
        else:
            assert len(unique_id) == COMM_ID_BYTES
            buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
            self._open(lib().kc_comm_create, int(rank), int(world), buf, int(device))
        self.rank, self.world = int(rank), int(world)

    @property
    def transport(self) -> str:
        return "shm" if lib().kc_comm_transport(self.h) == COMM_SHM else "rccl"

    def query(self):
        """(n_ranks, user_rank, device) as the transport itself reports them (RCCL: ncclCommCount /
        ncclCommUserRank / ncclCommCuDevice)."""
        n, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().kc_comm_query(self.h, C.byref(n), C.byref(r), C.byref(d)))
        return n.value, r.value, d.value


class DwaContext(_Owner, _Timed):
    """Owner of one kc_dwa context (one HIP stream, persistent device buffers)."""
    _kc, _timing_cap = "kc_dwa", 32

    def __init__(self, shape, dims, sensor_pos=(0, 0, 0), sensor_rot_xyzw=(0, 0, 0, 1), octree_res=0.1,
                 time_step=0.1, max_samples=1024, max_points=64, max_segment=512, max_obstacles=1024,
                 acc_limits=(1.0, 1.0, 1.0), device=0):
        p = DwaParams()
        p.shape = int(shape)
        d = list(dims) + [0.0] * (3 - len(dims))
        for i in range(3):
            p.dims[i] = float(np.float32(d[i]))
            p.sensor_pos[i] = float(np.float32(sensor_pos[i]))
            p.acc_limits[i] = float(np.float32(acc_limits[i]))
        p.ndims = len(dims)
        for i in range(4):
            p.sensor_rot_xyzw[i] = float(np.float32(sensor_rot_xyzw[i]))
        p.octree_res = float(octree_res)
        p.time_step = float(time_step)
        p.max_samples, p.max_points = int(max_samples), int(max_points)
        p.max_segment, p.max_obstacles = int(max_segment), int(max_obstacles)
        p.device = int(device)
        self.params = p
        self._open(lib().kc_dwa_create, C.byref(p))
        self._P = 0
        self._st = State()                      # reused by the per-cycle calls
        self._st_addr = C.addressof(self._st)
        self._n = _sz(0)
        self._n_addr = C.addressof(self._n)
        self._step = None

    # -- configuration ------------------------------------------------------
    def set_stream(self, stream_ptr):
        _check(lib().kc_dwa_set_stream(self.h, _vp(stream_ptr) if stream_ptr else None))

    def set_resolution(self, res):
        _check(lib().kc_dwa_set_resolution(self.h, float(res)))

    def set_option(self, name: str, value):
        _check(lib().kc_dwa_set_option(self.h, name.encode(), float(value)))

    def get_option(self, name: str) -> float:
        return _out(C.c_double, lib().kc_dwa_get_option, self.h, name.encode())

    def set_weights(self, w: Weights):
        _check(lib().kc_dwa_set_weights(self.h, C.byref(w)))

    def sample_window(self, ctr_type, limits: Limits, cur_vel, max_lin, max_ang, want_list=True):
        n = _sz(0)
        if want_list:
            cap = int(self.params.max_samples)
            vx, vy, om = np.zeros(cap), np.zeros(cap), np.zeros(cap)
            _check(lib().kc_dwa_sample_window(self.h, ctr_type, C.byref(limits), cur_vel[0], cur_vel[1],
                                              cur_vel[2], max_lin, max_ang, C.byref(n), _pd(vx), _pd(vy),
                                              _pd(om), cap))
            k = n.value
            return vx[:k].copy(), vy[:k].copy(), om[:k].copy()
        rc = _fast["kc_dwa_sample_window"](self.h, ctr_type, C.addressof(limits), cur_vel[0], cur_vel[1], cur_vel[2],
                                           max_lin, max_ang, self._n_addr, None, None, None, 0)
        if rc != KC_OK:
            _check(rc)
        return self._n.value

    def set_samples(self, vx, vy, omega):
        vx, vy, omega = _f64(vx), _f64(vy), _f64(omega)
        _check(lib().kc_dwa_set_samples(self.h, len(vx), _pd(vx), _pd(vy), _pd(omega)))

    def set_shard(self, first, count):
        _check(lib().kc_dwa_set_shard(self.h, int(first), int(count)))

    def set_shard_rule(self, rank, world, mode=SHARD_BLOCKS):
        """This context keeps rank `rank`'s share of every list it is given (mode < 0: all of it)."""
        _check(lib().kc_dwa_set_shard_rule(self.h, int(rank), int(world), int(mode)))

    def owns_sample(self, raw_index) -> bool:
        return bool(_out(C.c_int, lib().kc_dwa_owns_sample, self.h, int(raw_index)))

    def set_scan(self, state, ranges, angles, max_sensor_range=10.0):
        r, a = _f64(ranges), _f64(angles)
        st = State(*state)
        _check(lib().kc_dwa_set_scan(self.h, C.byref(st), _pd(r), _pd(a), len(r), float(max_sensor_range)))

    def _state(self, state):
        st = self._st
        st.x, st.y, st.yaw, st.speed = state
        return self._st_addr

    def set_points(self, state, xyz, max_sensor_range=10.0, global_frame=True):
        """updateSensorData(cloud, global_frame): world-frame points, or (global_frame=False) sensor-frame points."""
        p, addr = _addr32(xyz)
        if global_frame:
            rc = _fast["kc_dwa_set_points"](self.h, self._state(state), addr, p.size // 3, max_sensor_range)
        else:
            st = State(*state)
            rc = lib().kc_dwa_set_points_sensor_frame(self.h, C.byref(st), _pf(p), p.size // 3, float(max_sensor_range))
        if rc != KC_OK:
            _check(rc)

    def set_grid_device(self, state, dev_grid_ptr, grid_height, grid_width, resolution, central=None,
                        max_sensor_range=10.0):
        """OCCUPIED cells of a device-resident LocalMapper grid -> sensor data (8f rank 4)."""
        st = State(*state)
        if central is None:  # local_mapper.h:26-27
            central = (int(round(grid_height // 2)) - 1, int(round(grid_width // 2)) - 1)
        _check(lib().kc_dwa_set_grid_device(self.h, C.byref(st), _vp(dev_grid_ptr), int(grid_height),
                                            int(grid_width), float(np.float32(resolution)), int(central[0]),
                                            int(central[1]), float(max_sensor_range)))

    def set_grid_from_mapper(self, state, mapper, max_sensor_range=10.0):
        """Same, from a MapperContext: the scan may still be in flight (stream-ordered)."""
        st = State(*state)
        _check(lib().kc_dwa_set_grid_from_mapper(self.h, C.byref(st), mapper.h, float(max_sensor_range)))

    def set_worldmap(self, state, worldmap, max_sensor_range=10.0):
        """The occupied cells of a WorldMapContext within max_sensor_range of (state.x, state.y) -> sensor data, on the
        device (DESIGN.md 4.11 rules 16 to 19).  Same state as set_points with WorldMapContext.points' list."""
        st = State(*state)
        _check(lib().kc_dwa_set_worldmap(self.h, C.byref(st), None if worldmap is None else worldmap.h,
                                         float(np.float32(max_sensor_range))))

    def set_path(self, path_xyz, acc_at_point, total_length):
        """The whole interpolated reference path, resident on the device (once per path)."""
        pts = _f32(path_xyz).reshape(-1, 3)
        x, y, z = _f32(pts[:, 0]), _f32(pts[:, 1]), _f32(pts[:, 2])
        acc = _f32(acc_at_point)
        assert len(acc) == len(x)
        _check(lib().kc_dwa_set_path(self.h, _pf(x), _pf(y), _pf(z), _pf(acc), len(x),
                                     float(np.float32(total_length))))

    def set_tracked_window(self, start, size):
        """Tracked segment = points [start, start + size) of the resident path."""
        _check(lib().kc_dwa_set_tracked_window(self.h, int(start), int(size)))

    def set_tracked_segment(self, seg_xyz, acc_at_seg, ref_path_length):
        """Segment points as ONE (S, 3) array (kc_dwa_set_tracked_segment_xyz: no column copies here)."""
        seg, a_seg = _addr32(seg_xyz)
        acc, a_acc = _addr32(acc_at_seg)
        n = seg.size // 3
        assert acc.size == n
        rc = _fast["kc_dwa_set_tracked_segment_xyz"](self.h, a_seg, a_acc, n, float(np.float32(ref_path_length)))
        if rc != KC_OK:
            _check(rc)

    def set_tracked_segment_columns(self, x, y, z, acc_at_seg, ref_path_length):
        """The same from separate x / y / z arrays (what the C ABI takes: contiguous float32 arrays are passed
        where they lie, without the column copies of set_tracked_segment)."""
        (x, ax), (y, ay), (z, az), (acc, aa) = _addr32(x), _addr32(y), _addr32(z), _addr32(acc_at_seg)
        assert len(acc) == len(x)
        rc = _fast["kc_dwa_set_tracked_segment"](self.h, ax, ay, az, aa, len(x), float(np.float32(ref_path_length)))
        if rc != KC_OK:
            _check(rc)

    # -- cycle --------------------------------------------------------------
    def rollout(self, state, P):
        st = State(*state)
        self._P = int(P)
        _check(lib().kc_dwa_rollout(self.h, C.byref(st), int(P)))

    def check_poses(self, x, y, yaw):
        x, y, yaw = _f64(x), _f64(y), _f64(yaw)
        hit = np.zeros(len(x), np.uint8)
        _check(lib().kc_dwa_check_poses(self.h, _pd(x), _pd(y), _pd(yaw), len(x),
                                        hit.ctypes.data_as(C.POINTER(C.c_uint8))))
        return hit.astype(bool)

    def first_clear_command(self, state, vx, vy, omega, horizon, dt) -> int:
        """Index of the first (vx[i], vy[i], omega[i]) whose `horizon` poses rolled out
        from `state` with step (float)dt touch no occupied voxel, or -1 (one launch)."""
        vx, vy, omega = _f64(vx), _f64(vy), _f64(omega)
        if not (len(vx) == len(vy) == len(omega)):
            raise ValueError("vx, vy and omega must have the same length")
        st = state if isinstance(state, State) else State(*state)
        out = C.c_int64(-2)
        _check(lib().kc_dwa_first_clear_command(self.h, C.byref(st), _pd(vx), _pd(vy), _pd(omega), len(vx),
                                                int(horizon), float(dt), C.byref(out)))
        return int(out.value)

    def evaluate(self):
        _check(lib().kc_dwa_evaluate(self.h))

    def fetch_result(self) -> Result:
        r = Result()
        _check(lib().kc_dwa_fetch_result(self.h, C.byref(r)))
        return r

    def cycle(self, state, P) -> Result:
        self._P = int(P)
        r = Result()
        rc = _fast["kc_dwa_cycle"](self.h, self._state(state), self._P, C.addressof(r))
        if rc != KC_OK:
            _check(rc)
        return r

    def find_best_path(self, state, P, *, window=None, points=None, scan=None, max_sensor_range=10.0,
                       segment=None) -> Result:
        """One reference controller cycle in ONE call (kc_dwa_find_best_path = DWA::findBestPath, dwa.h:183-230):
        window = (ctr_type, Limits, (vx, vy, omega), max_linear_samples, max_angular_samples), points = (n, 3)
        float32 array or scan = (ranges, angles) float64 arrays, segment = (seg_xyz (S, 3) float32, acc_at_seg,
        ref_path_length).  An omitted part keeps what the context holds.  The arrays of the previous call are
        recognised by identity (same objects: their addresses are reused)."""
        si = self._step
        if si is None:
            si = self._step = StepInputs()
            self._step_addr = C.addressof(si)
            self._step_keep = [None] * 6   # the arrays whose addresses sit in the structure (kept alive)
        keep = self._step_keep
        if window is not None:
            ctr, lim, cur, ml, ma = window
            if keep[5] is not lim:
                keep[5] = lim
                si.limits = C.addressof(lim)
            si.ctr_type, si.max_linear_samples, si.max_angular_samples = ctr, ml, ma
            si.cur_vx, si.cur_vy, si.cur_omega = cur
        else:
            si.limits = None
            keep[5] = None
        if points is not None:
            if keep[0] is not points:
                p, addr = _addr32(points)
                keep[0] = points if p is points else None  # (a converted copy lives only for this call)
                self._step_tmp = p
                si.points_xyz, si.n_points = addr, p.size // 3
                si.scan_ranges = si.scan_angles = None
        elif scan is not None:
            r, ang = _f64(scan[0]), _f64(scan[1])
            self._step_tmp = (r, ang)
            keep[0] = None
            si.points_xyz = None
            si.scan_ranges, si.scan_angles, si.n_beams = r.ctypes.data, ang.ctypes.data, len(r)
        else:
            si.points_xyz = si.scan_ranges = si.scan_angles = None
            keep[0] = None
        si.max_sensor_range = max_sensor_range
        if segment is not None:
            seg, acc, ref_len = segment
            if keep[1] is not seg or keep[2] is not acc:
                s2, a_seg = _addr32(seg)
                a2, a_acc = _addr32(acc)
                keep[1] = seg if s2 is seg else None
                keep[2] = acc if a2 is acc else None
                self._step_tmp2 = (s2, a2)
                si.seg_xyz, si.acc_at_seg, si.seg_size = a_seg, a_acc, s2.size // 3
                si.seg_x = si.seg_y = si.seg_z = None
            si.ref_path_length = ref_len
        else:
            si.seg_size = 0
            keep[1] = keep[2] = None
        self._P = si.num_points = int(P)
        r = Result()
        rc = _fast["kc_dwa_find_best_path"](self.h, self._state(state), self._step_addr, C.addressof(r))
        if rc != KC_OK:
            _check(rc)
        return r

    def get_best(self):
        P = self._P
        px, py = np.zeros(P, np.float32), np.zeros(P, np.float32)
        v = [np.zeros(P - 1, np.float32) for _ in range(3)]
        _check(lib().kc_dwa_get_best(self.h, _pf(px), _pf(py), _pf(v[0]), _pf(v[1]), _pf(v[2])))
        return px, py, v

    def get_samples(self, with_costs=False, with_paths=True):
        path = (np.float32, (self._P,)) if with_paths else None
        px, py, raw, costs = _fill(lib().kc_dwa_get_samples, self.h,
                                   [path, path, (np.int32, ()), (np.float32, ()) if with_costs else None])
        return (px, py, raw, costs) if with_costs else (px, py, raw)

    def get_freeze_steps(self):
        return _fill(lib().kc_dwa_get_freeze_steps, self.h, [(np.int32, ())])[0]

    def get_sample_velocity(self, raw_index):
        vx, vy, om = C.c_double(0), C.c_double(0), C.c_double(0)
        _check(lib().kc_dwa_get_sample_velocity(self.h, int(raw_index), C.byref(vx), C.byref(vy), C.byref(om)))
        return vx.value, vy.value, om.value

    def cost_evaluate(self, paths_x, paths_y, vel=None):
        px, py = _f32(paths_x), _f32(paths_y)
        N, P = px.shape
        self._P = P
        costs = np.zeros(max(N, 1), np.float32)
        r = Result()
        v = [_f32(a) for a in vel] if vel is not None else [None, None, None]
        _check(lib().kc_cost_evaluate(self.h, _pf(px), _pf(py), _pf(v[0]), _pf(v[1]), _pf(v[2]), N, P,
                                      _pf(costs), C.byref(r)))
        return r, costs[:N]

    def cost_upload(self, paths_x, paths_y, vel=None):
        px, py = _f32(paths_x), _f32(paths_y)
        N, P = px.shape
        self._P, self._N = P, N
        v = [_f32(a) for a in vel] if vel is not None else [None, None, None]
        _check(lib().kc_cost_upload(self.h, _pf(px), _pf(py), _pf(v[0]), _pf(v[1]), _pf(v[2]), N, P))

    def cost_evaluate_resident(self, with_costs=True):
        r = Result()
        costs = np.zeros(max(self._N, 1), np.float32) if with_costs else None
        _check(lib().kc_cost_evaluate_resident(self.h, _pf(costs), C.byref(r)))
        return (r, costs[:self._N]) if with_costs else r

    def allreduce_best(self, comm: "Comm"):
        """ONE ncclAllReduce(int64, min) of the key record + hand-off of the reduced record."""
        _check(lib().kc_dwa_allreduce_best(self.h, comm.h))

    def cycle_sharded(self, comm: "Comm", state, P) -> Result:
        st = State(*state)
        self._P = int(P)
        r = Result()
        _check(lib().kc_dwa_cycle_sharded(self.h, comm.h, C.byref(st), int(P), C.byref(r)))
        return r

    def exchange_best(self, comm: "Comm", found, cost, raw_index, status=0) -> Result:
        """The exchange of a sharded cycle whose last cost terms the HOST added (custom cost callbacks): this
        rank's own best {found, cost, global raw index} in, the global result out (kc_dwa_exchange_best)."""
        r = Result()
        _check(lib().kc_dwa_exchange_best(self.h, comm.h, int(status), int(bool(found)), float(np.float32(cost)),
                                          int(raw_index), C.byref(r)))
        return r

    def global_index(self, comm: "Comm", raw_index) -> int:
        return _out(C.c_int64, lib().kc_dwa_global_index, self.h, comm.h, int(raw_index))

    def publish_result(self):
        """After an in-place reduction of the device record: hand it to the host
        through pinned memory (fetch_result then returns the reduced key)."""
        _check(lib().kc_dwa_publish_result(self.h))

    def result_device_ptr(self) -> int:
        return _out(_vp, lib().kc_dwa_result_device, self.h)

    def count_admissible_before(self, raw_index) -> int:
        return _out(C.c_int64, lib().kc_dwa_count_admissible_before, self.h, int(raw_index))


class MapperContext(_Owner, _Timed):
    """Owner of one kc_mapper context (LocalMapper scan -> grid)."""
    _kc = "kc_mapper"

    def __init__(self, grid_height, grid_width, resolution, laserscan_position=(0, 0, 0),
                 laserscan_orientation=0.0, max_scan_size=4096, device=0):
        pos = _f32(laserscan_position)
        self.H, self.W = int(grid_height), int(grid_width)
        self._open(lib().kc_mapper_create, self.H, self.W, float(np.float32(resolution)), _pf(pos),
                   float(np.float32(laserscan_orientation)), int(max_scan_size), int(device))

    def set_stream(self, stream_ptr):
        _check(lib().kc_mapper_set_stream(self.h, _vp(stream_ptr) if stream_ptr else None))

    def scan_to_grid(self, angles, ranges):
        """-> int32 [H, W] with the Eigen column-major storage undone."""
        a, r = _f64(angles), _f64(ranges)
        g = np.empty(self.H * self.W, np.int32)
        _check(lib().kc_mapper_scan_to_grid(self.h, _pd(a), _pd(r), len(a), g.ctypes.data_as(_ip)))
        return g.reshape(self.W, self.H).T

    def scan_to_grid_device(self, angles, ranges):
        a, r = _f64(angles), _f64(ranges)
        _check(lib().kc_mapper_scan_to_grid_device(self.h, _pd(a), _pd(r), len(a)))

    # ---- M3: Bayesian update (LocalMapper's second ctor) ----------------------
    def enable_bayes(self, p_prior=0.5, p_occupied=0.6, p_empty=0.4, range_sure=1.0, range_max=20.0,
                     wall_size=0.2):
        params = (C.c_float * 6)(*[float(np.float32(v)) for v in
                                   (p_prior, p_occupied, p_empty, range_sure, range_max, wall_size)])
        _check(lib().kc_mapper_enable_bayes(self.h, C.cast(params, C.c_void_p)))

    def scan_to_grid_baysian(self, angles, ranges):
        """-> (int32 [H, W] occupancy, float32 [H, W] probabilities)."""
        a, r = _f64(angles), _f64(ranges)
        g = np.empty(self.H * self.W, np.int32)
        pr = np.empty(self.H * self.W, np.float32)
        _check(lib().kc_mapper_scan_to_grid_bayes(self.h, _pd(a), _pd(r), len(a), g.ctypes.data_as(_ip),
                                                  _pf(pr)))
        return g.reshape(self.W, self.H).T, pr.reshape(self.W, self.H).T

    def scan_to_grid_baysian_device(self, angles, ranges):
        a, r = _f64(angles), _f64(ranges)
        _check(lib().kc_mapper_scan_to_grid_bayes_device(self.h, _pd(a), _pd(r), len(a)))

    def prob_device_ptrs(self):
        p, q = _vp(), _vp()
        _check(lib().kc_mapper_prob_device(self.h, C.byref(p), C.byref(q)))
        return p.value, q.value

    def get_previous_grid_in_current_pose(self, position, orientation):
        pos = _f32(np.asarray(position, np.float32)[:2])
        _check(lib().kc_mapper_warp_previous(self.h, _pf(pos), float(orientation)))

    def previous_prob(self):
        pr = np.empty(self.H * self.W, np.float32)
        _check(lib().kc_mapper_get_previous_prob(self.h, _pf(pr)))
        return pr.reshape(self.W, self.H).T

    def set_previous_prob(self, prob=None):
        """prob [H, W] -> previous grid; None feeds the last scan's probabilities back (device copy)."""
        if prob is None:
            _check(lib().kc_mapper_set_previous_prob(self.h, None))
            return
        flat = np.ascontiguousarray(np.asarray(prob, np.float32).T).reshape(-1)
        if flat.size != self.H * self.W:
            raise ValueError("previous grid must be [grid_height, grid_width]")
        _check(lib().kc_mapper_set_previous_prob(self.h, _pf(flat)))

    def sync(self):
        _check(lib().kc_mapper_sync(self.h))

    def grid_device_ptr(self) -> int:
        return _out(_vp, lib().kc_mapper_grid_device, self.h)


class CloudContext(_Owner, _Timed, _StreamOrdered):
    """Owner of one kc_cloud context (raw point cloud -> laserscan)."""
    _kc = "kc_cloud"

    def __init__(self, max_bytes=1 << 20, max_bins=4096, device=0):
        self._open(lib().kc_cloud_create, int(max_bytes), int(max_bins), int(device))

    def to_laserscan(self, data, point_step, row_step, height, width, x_offset, y_offset, z_offset,
                     max_range, min_z, max_z, angle_step=None, num_bins=None, device_ptr=None, nbytes=None,
                     field_type=7):
        """pointCloudToLaserScanFromRaw: (ranges, angles) with angle_step,
        ranges with num_bins.  `data`: bytes / int8 array on the host, or pass
        device_ptr + nbytes for a buffer that already lives on the device."""
        by_step = angle_step is not None
        nb = int(np.ceil(2.0 * np.pi / angle_step)) if by_step else int(num_bins)
        cap = max(nb, 1)
        ranges = np.zeros(cap, np.float64)
        angles = np.zeros(cap, np.float64)
        n = _sz(0)
        if device_ptr is not None:
            ptr, size, on_dev = int(device_ptr), int(nbytes), 1
        else:
            buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.int8)
                                       if not isinstance(data, np.ndarray) else data.view(np.int8).reshape(-1))
            ptr, size, on_dev = buf.ctypes.data, buf.size, 0
        _check(lib().kc_cloud_to_laserscan_typed(self.h, ptr, size, on_dev, int(point_step), int(row_step), int(height),
                                                 int(width), int(x_offset), int(y_offset), int(z_offset), int(field_type),
                                                 float(max_range), float(min_z), float(max_z),
                                                 float(angle_step) if by_step else 0.0, nb, _pd(ranges), _pd(angles),
                                                 cap, C.byref(n)))
        return (ranges[:n.value], angles[:n.value]) if by_step else ranges[:n.value]

    def occupancy_grid(self, points, grid_resolution, z_ground_limit, robot_height, device_ptr=None, n_points=None,
                       point_step=12, offsets=(0, 4, 8), nbytes=None, to_host=True):
        """The two loops of readPCDToOccupancyGrid: (grid, origin), grid an int8 (cells_x, cells_y) array with
        grid[i, j] the cell (i, j), origin [min_x, min_y, 0].  `points`: an (N, 3) float32 array on the host,
        or raw records (bytes / int8 array with point_step, offsets and n_points); or pass device_ptr, n_points
        (and nbytes) for a cloud that already lives on the device.  to_host=False runs the passes and returns
        (device address of the grid, (cells_x, cells_y), origin) instead."""
        with np.errstate(over="ignore"):
            res = float(np.float32(grid_resolution))  # what the C ABI receives
        if not (res > 0.0 and np.isfinite(res)):
            raise ValueError("grid_resolution must be a positive finite float")
        step = int(point_step)
        if device_ptr is not None:
            n = int(n_points)
            ptr, on_dev = int(device_ptr), 1
            size = int(nbytes) if nbytes is not None else n * step
        else:
            if isinstance(points, np.ndarray) and points.dtype != np.int8:
                if points.ndim != 2 or points.shape[1] != 3:
                    raise ValueError("expected an (N, 3) array of points")
                buf = _f32(points)
                n = buf.shape[0] if n_points is None else int(n_points)
            else:
                buf = np.ascontiguousarray(np.frombuffer(bytes(points), dtype=np.int8)
                                           if not isinstance(points, np.ndarray) else points.reshape(-1))
                n = buf.size // step if n_points is None else int(n_points)
            ptr, size, on_dev = buf.ctypes.data, buf.nbytes, 0
        origin = np.zeros(3, np.float32)
        cx, cy = C.c_int(0), C.c_int(0)
        _check(lib().kc_cloud_grid_extent(self.h, ptr, size, on_dev, step, n, int(offsets[0]), int(offsets[1]),
                                          int(offsets[2]), res, _pf(origin), C.byref(cx), C.byref(cy)))
        if not to_host:
            dev = _out(_vp, lib().kc_cloud_grid_device, self.h, float(z_ground_limit), float(robot_height))
            return dev or 0, (cx.value, cy.value), origin
        grid = np.empty((cx.value, cy.value), np.int8, order="F")
        _check(lib().kc_cloud_grid_fill(self.h, float(z_ground_limit), float(robot_height), grid.ctypes.data, grid.size))
        return grid, origin

    def last_rebinned(self) -> int:
        return _out(_sz, lib().kc_cloud_last_rebinned, self.h)


class ZoneContext(_Owner):
    """Owner of one kc_zone context (CriticalZoneChecker)."""
    _kc = "kc_zone"

    def __init__(self, shape, dims, sensor_pos, sensor_rot_xyzw, critical_angle, critical_distance,
                 slowdown_distance, angles, min_height, max_height, range_max, device=0):
        d, sp, sr = _f32(dims), _f32(sensor_pos), _f32(sensor_rot_xyzw)
        a = _f64(angles)
        self.n = len(a)
        self._open(lib().kc_zone_create, int(shape), _pf(d), len(d), _pf(sp), _pf(sr), float(np.float32(critical_angle)),
                   float(np.float32(critical_distance)), float(np.float32(slowdown_distance)), _pd(a), len(a),
                   float(np.float32(min_height)), float(np.float32(max_height)), float(np.float32(range_max)), int(device))

    def check(self, ranges, forward) -> float:
        r = _f64(ranges)
        return float(_out(C.c_float, lib().kc_zone_check, self.h, _pd(r), len(r), int(bool(forward))))

    def check_worldmap(self, worldmap: "WorldMapContext", pose, forward, unknown_blocks=False, real=None,
                       flags=None) -> float:
        """check() on the virtual scan of `worldmap` at the scan frame's `pose` ((x, y, yaw) or a WorldMapPose) over the
        preset angles and range_max (DESIGN.md 4.11 rules 20 to 27).  real: the preset's count of present ranges to
        merge by rule 27."""
        q = None if real is None else _f64(real).reshape(-1)
        if q is not None and len(q) != self.n:
            raise ValueError(f"{len(q)} present ranges for a preset of {self.n} angles")
        p = worldmap._pose(pose)
        return float(_out(C.c_float, lib().kc_zone_check_worldmap, self.h, worldmap.h, C.byref(p),
                          _scan_flags(unknown_blocks, flags), _pd(q), int(bool(forward))))

    def check_cloud(self, data, point_step, row_step, height, width, x_offset, y_offset, z_offset, forward,
                    field_type=7) -> float:
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.int8) if not isinstance(data, np.ndarray)
                                   else data.view(np.int8).reshape(-1))
        return float(_out(C.c_float, lib().kc_zone_check_cloud_typed, self.h, buf.ctypes.data, buf.size, int(point_step),
                          int(row_step), int(height), int(width), int(x_offset), int(y_offset), int(z_offset),
                          int(field_type), int(bool(forward))))

    def indices(self, forward):
        out = (C.c_int64 * max(self.n, 1))()
        n = _sz(0)
        _check(lib().kc_zone_indices(self.h, int(bool(forward)), out, self.n, C.byref(n)))
        return np.array(out[:n.value], dtype=np.int64)


class DepthContext(_Owner, _Timed, _StreamOrdered):
    """Owner of one kc_depth context (DepthDetector: 2-D boxes -> 3-D boxes)."""
    _kc = "kc_depth"

    def __init__(self, depth_range, camera_in_body_translation, camera_in_body_rotation, focal_length,
                 principal_point, depth_conversion_factor=1e-3, device=0):
        dr, t, q = _f32(depth_range), _f32(camera_in_body_translation), _f32(camera_in_body_rotation)
        f, p = _f32(focal_length), _f32(principal_point)
        if dr.shape != (2,) or t.shape != (3,) or q.shape != (4,) or f.shape != (2,) or p.shape != (2,):
            raise ValueError("depth_range (2), translation (3), rotation xyzw (4), focal (2), principal (2)")
        self._open(lib().kc_depth_create, _pf(dr), _pf(t), _pf(q), _pf(f), _pf(p),
                   float(np.float32(depth_conversion_factor)), int(device))

    @staticmethod
    def _frame(img, device_ptr, shape, strides):
        """(address, on_device, rows, cols, row_stride, col_stride) in elements; `img` is kept alive by the caller."""
        if device_ptr is not None:
            rows, cols = (int(v) for v in shape)
            rs, cs = (int(v) for v in strides) if strides is not None else (cols, 1)
            return int(device_ptr), 1, rows, cols, rs, cs
        if not isinstance(img, np.ndarray) or img.dtype != np.uint16:
            raise TypeError("the depth frame must be a uint16 numpy array")
        if img.ndim != 2:
            raise ValueError(f"the depth frame must be 2-D (H, W), got shape {img.shape}")
        rs, cs = (s // 2 for s in img.strides)
        return img.__array_interface__["data"][0], 0, img.shape[0], img.shape[1], rs, cs

    @staticmethod
    def _boxes(boxes):
        b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        return b, b.ctypes.data_as(_ip)

    def boxes(self, img, boxes, state=None, device_ptr=None, shape=None, strides=None):
        """(centres [m, 3], sizes [m, 3], kept input indices [m]) of the kept boxes.  boxes: [n, 4] of
        (top.x, top.y, size.x, size.y); state: (x, y, yaw) or None to keep the previous one."""
        addr, on_dev, rows, cols, rs, cs = self._frame(img, device_ptr, shape, strides)
        b, pb = self._boxes(boxes)
        n = len(b)
        out = np.zeros((max(n, 1), 6), np.float32)
        idx = np.zeros(max(n, 1), np.int32)
        st = None if state is None else _f64(state)
        m = _sz(0)
        _check(lib().kc_depth_boxes(self.h, addr, on_dev, rows, cols, rs, cs, pb, n, _pd(st), _pf(out),
                                    idx.ctypes.data_as(_ip), max(n, 1), C.byref(m)))
        k = m.value
        return out[:k, :3].copy(), out[:k, 3:].copy(), idx[:k].copy()

    def box_stats(self, img, boxes, device_ptr=None, shape=None, strides=None):
        """(count [n] int64, [n, 4] float32 of median, mad, min_d, max_d)."""
        addr, on_dev, rows, cols, rs, cs = self._frame(img, device_ptr, shape, strides)
        b, pb = self._boxes(boxes)
        n = len(b)
        cnt = np.zeros(max(n, 1), np.int64)
        st = np.zeros((max(n, 1), 4), np.float32)
        _check(lib().kc_depth_box_stats(self.h, addr, on_dev, rows, cols, rs, cs, pb, n,
                                        cnt.ctypes.data_as(C.POINTER(C.c_int64)), _pf(st)))
        return cnt[:n], st[:n]

    def last_upload(self) -> int:
        return _out(_sz, lib().kc_depth_last_upload, self.h)


class DvzContext(_Owner):
    """Owner of one kc_dvz context (DeformableVirtualZone.get_total_deformation: one launch per call)."""
    _kc = "kc_dvz"

    def __init__(self, max_beams=4096, device=0):
        if int(max_beams) < 0:
            raise ValueError(f"max_beams must be non-negative, got {max_beams}")
        self.max_beams = int(max_beams)
        self._open(lib().kc_dvz_create, int(device), self.max_beams)

    def deform(self, zone, angles, ranges, radii=False):
        """(total, orientation_sum, n_deformed) over the beams, plus the per-beam deformed radii when `radii`.
        zone: a DvzZone or (major_radius, minor_radius, center_shift_x, center_shift_y, ori_shift)."""
        z = zone if isinstance(zone, DvzZone) else DvzZone(*(float(v) for v in zone))
        a, r = _f64(angles).reshape(-1), _f64(ranges).reshape(-1)
        if len(a) != len(r):
            raise ValueError(f"{len(a)} angles and {len(r)} ranges")
        out = (C.c_double * 3)()
        rad = np.zeros(max(len(a), 1)) if radii else None
        _check(lib().kc_dvz_deform(self.h, C.byref(z), _pd(a), _pd(r), len(a), out, _pd(rad)))
        res = (float(out[0]), float(out[1]), int(out[2]))
        return res + (rad[:len(a)],) if radii else res

    def deform_worldmap(self, zone, worldmap: "WorldMapContext", pose, angles, range_max, unknown_blocks=False, real=None,
                        radii=False, flags=None):
        """deform() on the virtual scan of `worldmap` at `pose` ((x, y, yaw) or a WorldMapPose; DESIGN.md 4.11 rules 20 to
        27), queued on this context's stream without the ranges leaving the device.  real: present ranges to merge by
        rule 27.  -> (total, orientation_sum, n_deformed, ranges[, radii])."""
        z = zone if isinstance(zone, DvzZone) else DvzZone(*(float(v) for v in zone))
        a = _f64(angles).reshape(-1)
        q = None if real is None else _f64(real).reshape(-1)
        if q is not None and len(q) != len(a):
            raise ValueError(f"{len(a)} angles and {len(q)} present ranges")
        p = worldmap._pose(pose)
        out = (C.c_double * 3)()
        rad = np.zeros(max(len(a), 1)) if radii else None
        rng = np.zeros(max(len(a), 1))
        _check(lib().kc_dvz_deform_worldmap(self.h, C.byref(z), worldmap.h, C.byref(p), _pd(a), len(a),
                                            float(np.float32(range_max)), _scan_flags(unknown_blocks, flags), _pd(q), out,
                                            _pd(rad), _pd(rng)))
        res = (float(out[0]), float(out[1]), int(out[2]), rng[:len(a)])
        return res + (rad[:len(a)],) if radii else res


PLAN_FOUND, PLAN_START_OUTSIDE, PLAN_GOAL_OUTSIDE, PLAN_START_INVALID, PLAN_GOAL_INVALID, PLAN_UNREACHABLE = range(6)
PLAN_NO_FRONTIER = 6
# kc_planner_frontier, field for field
PLAN_FRONTIER_DTYPE = np.dtype([("sum_i", np.uint64), ("sum_j", np.uint64), ("size", np.uint32), ("root", np.uint32),
                                ("cost", np.uint32), ("entry_i", np.int32), ("entry_j", np.int32), ("reserved_", np.uint32)])
PLAN_INF = 0xFFFFFFFF
PLAN_CLEAR_FAR = 0xFFFF
PLAN_MAX_SPAN = 1024
PLAN_MAX_TURN_CELLS = 8
PLAN_MAX_REVERSE_WEIGHT = 16


class PlannerContext(_Owner, _StreamOrdered):
    """Owner of one kc_planner context (grid planner).  Works in cells: a grid is an array
    g[i, j] of (width, height) cells, i along x; world coordinates are the business of kompass_cpp.planning."""
    _kc = "kc_planner"

    def __init__(self, device=0):
        self.shape = (0, 0)
        self._open(lib().kc_planner_create, int(device))

    def set_grid(self, grid):
        """grid[i, j]: an int32 or int8 (width, height) array on the host, any memory order."""
        g = np.asarray(grid)
        if g.ndim != 2 or g.dtype not in (np.int32, np.int8):
            raise ValueError("expected a 2-D int32 or int8 grid")
        g = np.asfortranarray(g)  # cell (i, j) at i + j * width
        _check(lib().kc_planner_set_grid_host(self.h, g.ctypes.data, g.itemsize, g.shape[0], g.shape[1]))
        self.shape = g.shape

    def set_grid_device(self, device_ptr, width, height, elem_bytes=4):
        """A finished grid on the context's device (MapperContext.grid_device_ptr after sync: int32, width =
        grid_height, height = grid_width; CloudContext.occupancy_grid(to_host=False): int8)."""
        _check(lib().kc_planner_set_grid_device(self.h, int(device_ptr), int(elem_bytes), int(width), int(height)))
        self.shape = (int(width), int(height))

    def solve(self, start, goal, r2=0, allow_unknown=True):
        """-> (status, cost, passes): PLAN_* status, field[start] in units of 10 per straight step."""
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        st, cost, passes = C.c_int(-1), C.c_uint32(0), C.c_int(0)
        _check(lib().kc_planner_solve(self.h, s, g, int(r2), int(bool(allow_unknown)), C.byref(st), C.byref(cost),
                                      C.byref(passes)))
        return st.value, cost.value, passes.value

    def field(self):
        """(field uint32 [width, height], valid bool [width, height]) of the last solve."""
        w, h = self.shape
        f = np.empty((w, h), np.uint32, order="F")
        v = np.empty((w, h), np.uint8, order="F")
        _check(lib().kc_planner_get_field(self.h, f.ctypes.data, v.ctypes.data, f.size))
        return f, v.astype(bool)

    def field_device(self):
        """(device pointer, width, height, stream) of the kept cost field where it lies (kc_planner_field_device): uint32,
        cell (i, j) at i + j * width.  Holds until the next solve-type call.  Raises KompassHipError (KC_ERR_STATE) unless
        the last solve-type call was solve or replan."""
        f, w, h, st = C.c_void_p(None), C.c_int(0), C.c_int(0), C.c_void_p(None)
        _check(lib().kc_planner_field_device(self.h, C.byref(f), C.byref(w), C.byref(h), C.byref(st)))
        return int(f.value or 0), w.value, h.value, int(st.value or 0)

    def path(self):
        """(n, 2) int32 cells (i, j) from the start to the goal; n = 0 when the last solve found none."""
        return _fill(lib().kc_planner_get_path, self.h, [(np.int32, (2,))])[0]

    def set_clearance_cost(self, c2, table=None):
        """The clearance cost of rules 6 to 8: table[d2] for d2 = 0 .. c2 is the surcharge of a cell whose nearest
        blocking cell lies at squared distance d2.  c2 = 0 (or no table) switches it off.  Forgets the last solve."""
        if table is None or int(c2) == 0:
            _check(lib().kc_planner_set_clearance_cost(self.h, int(c2), None, 0))
            return
        t = np.ascontiguousarray(table)
        if t.ndim != 1 or t.dtype.kind not in "iu" or (t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF)):
            raise ValueError("expected a 1-D table of integers that fit uint32")
        t = t.astype(np.uint32)
        _check(lib().kc_planner_set_clearance_cost(self.h, int(c2), t.ctypes.data, t.size))

    def clearance(self):
        """(clear2 uint16 [width, height], penalty uint32 [width, height]) of the last solve; raises with the
        clearance cost off."""
        w, h = self.shape
        c = np.empty((w, h), np.uint16, order="F")
        p = np.empty((w, h), np.uint32, order="F")
        _check(lib().kc_planner_get_clearance(self.h, c.ctypes.data, p.ctypes.data, c.size))
        return c, p

    def path_clearance(self):
        """The smallest clear2 along the last path, both ends included (PLAN_CLEAR_FAR: nothing within reach)."""
        return _out(C.c_uint32, lib().kc_planner_path_clearance, self.h)

    def shortcut(self, max_span=128):
        """The any-angle path of rules 9 to 12 over the last path: (cells (k, 2) int32, indices (k,) int32 into
        path(), min_clear2).  From each kept cell the farthest of the next max_span cells in line of sight is kept;
        min_clear2 is the smallest clear2 the kept segments touch (PLAN_CLEAR_FAR with the clearance cost off)."""
        n, v = _sz(0), C.c_uint32(0)
        _check(lib().kc_planner_shortcut(self.h, int(max_span), C.byref(n), C.byref(v)))
        cells, idx = np.empty((n.value, 2), np.int32), np.empty(n.value, np.int32)
        _check(lib().kc_planner_get_shortcut(self.h, cells.ctypes.data, idx.ctypes.data, n.value, C.byref(n)))
        return cells, idx, v.value

    def set_oriented(self, a2, b2=0, turn10=10):
        """The oriented box footprint of rules 13 to 18: a2 / b2 the squared half length / half width in cells,
        turn10 the cost of a turn by one class (a straight step is 10).  a2 = 0 switches it off.  Forgets the last
        solve."""
        _check(lib().kc_planner_set_oriented(self.h, int(a2), int(b2), int(turn10)))

    def solve_oriented(self, start, start_class, goal, allow_unknown=True):
        """-> (status, cost, passes) for the state (start cell, start class): cost = field[start_class][start], the
        turns included."""
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        st, cost, passes = C.c_int(-1), C.c_uint32(0), C.c_int(0)
        _check(lib().kc_planner_solve_oriented(self.h, s, int(start_class), g, int(bool(allow_unknown)), C.byref(st),
                                               C.byref(cost), C.byref(passes)))
        return st.value, cost.value, passes.value

    def oriented_field(self):
        """(field uint32 [4, width, height], valid bool [4, width, height], turn_valid bool [width, height]) of the
        last oriented solve."""
        w, h = self.shape
        f = np.empty((4, h, w), np.uint32)   # layer k, then the grid's layout: cell (i, j) at i + j * width
        v = np.empty((w, h), np.uint8, order="F")
        t = np.empty((w, h), np.uint8, order="F")
        _check(lib().kc_planner_get_oriented_field(self.h, f.ctypes.data, v.ctypes.data, t.ctypes.data, v.size))
        valid = np.stack([(v >> k & 1).astype(bool) for k in range(4)])
        return f.transpose(0, 2, 1), valid, t.astype(bool)

    def oriented_path(self):
        """(n, 3) int32 states (i, j, k) of the walk from (start, start class) to the goal; n = 0 when the last
        oriented solve found none.  path() gives its cells with the repeated cell of a turn collapsed."""
        return _fill(lib().kc_planner_get_oriented_path, self.h, [(np.int32, (3,))])[0]

    def set_car(self, turn_cells, reverse_weight=0, a2=0, b2=0):
        """Car motion of rules 27 to 36: turn_cells the legs of a 45-degree arc in cells (1 .. PLAN_MAX_TURN_CELLS),
        reverse_weight the factor on backward primitives (0: none, up to 16), a2 / b2 the box footprint as
        set_oriented's (0, 0: the disc of solve_car's r2).  turn_cells = 0 switches it off.  Forgets the last solve."""
        _check(lib().kc_planner_set_car(self.h, int(turn_cells), int(reverse_weight), int(a2), int(b2)))

    def solve_car(self, start, start_heading, goal, goal_heading=-1, r2=0, allow_unknown=True):
        """-> (status, cost, passes) for the state (start cell, start heading 0 .. 7) to (goal cell, goal heading; -1:
        any): cost = field[start_heading][start]."""
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        st, cost, passes = C.c_int(-1), C.c_uint32(0), C.c_int(0)
        _check(lib().kc_planner_solve_car(self.h, s, int(start_heading), g, int(goal_heading), int(r2),
                                          int(bool(allow_unknown)), C.byref(st), C.byref(cost), C.byref(passes)))
        return st.value, cost.value, passes.value

    def car_field(self):
        """(field uint32 [8, width, height], moves uint8 [8, width, height] (bit p = primitive p of S, L, R, B, BL, BR
        allowed), valid bool [8, width, height]) of the last car solve."""
        w, h = self.shape
        f = np.empty((8, h, w), np.uint32)   # layer h, then the grid's layout: cell (i, j) at i + j * width
        m = np.empty((8, h, w), np.uint8)
        v = np.empty((w, h), np.uint8, order="F")
        _check(lib().kc_planner_get_car_field(self.h, f.ctypes.data, m.ctypes.data, v.ctypes.data, v.size))
        valid = np.stack([(v >> k & 1).astype(bool) for k in range(8)])
        return f.transpose(0, 2, 1), m.transpose(0, 2, 1), valid

    def car_path(self):
        """(states (m, 3) int32 (i, j, h), one per primitive boundary, moves (m - 1,) int32 primitive ids) of the last
        car solve; m = 0 when it found none.  path() gives every unit step of every primitive."""
        n = _sz(0)
        _check(lib().kc_planner_get_car_path(self.h, None, None, 0, C.byref(n)))
        states, moves = np.empty((n.value, 3), np.int32), np.empty(max(n.value - 1, 0), np.int32)
        if n.value:
            _check(lib().kc_planner_get_car_path(self.h, states.ctypes.data, moves.ctypes.data, n.value, C.byref(n)))
        return states, moves

    def car_info(self):
        """(turn_cells, reverse_weight, (maps + moves ms, field ms, walk ms)) of the mode and the last car solve."""
        n, rw, ms = C.c_int(0), C.c_uint32(0), (C.c_float * 3)()
        _check(lib().kc_planner_car_info(self.h, C.byref(n), C.byref(rw), ms))
        return n.value, rw.value, tuple(float(v) for v in ms)

    def replan(self, start, goal, r2=0, allow_unknown=True):
        """solve() from the field the context kept (rules 19 and 20): the same outputs bit for bit, the passes only
        over what a grid set since the last solve changed, none when only the start moved.  A full solve when
        there is no kept field or goal, r2, allow_unknown, the clearance table or the shape differ.
        -> (status, cost, passes)."""
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        st, cost, passes = C.c_int(-1), C.c_uint32(0), C.c_int(0)
        _check(lib().kc_planner_replan(self.h, s, g, int(r2), int(bool(allow_unknown)), C.byref(st), C.byref(cost),
                                       C.byref(passes)))
        return st.value, cost.value, passes.value

    def replan_info(self):
        """(replanned, threshold, touched, active_tiles) of the last replan(): whether it kept a field, rule 19's T
        (PLAN_INF: nothing to roll back), the touched cells and the tiles a pass ran over."""
        kept, t, touched, tiles = C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().kc_planner_replan_info(self.h, C.byref(kept), C.byref(t), C.byref(touched), C.byref(tiles)))
        return bool(kept.value), t.value, touched.value, tiles.value

    def explore(self, robot, r2=0, min_cost=0, min_size=1):
        """The reachable frontiers of the known map, nearest first (rules 21 to 26): frontier cells are explore-valid
        cells (no occupied cell within r2, not unknown) with min_cost <= field < INF from the robot's cell and an
        unknown orthogonal neighbour; a frontier is an 8-connected component of them, kept from min_size cells on.
        -> (status, components, kept, field passes, label passes); status PLAN_FOUND, PLAN_NO_FRONTIER,
        PLAN_START_OUTSIDE or PLAN_START_INVALID.  field() then gives the explore field and validity."""
        cell = (C.c_int32 * 2)(int(robot[0]), int(robot[1]))
        st, comps, kept, passes, lpasses = C.c_int(-1), C.c_uint32(0), _sz(0), C.c_int(0), C.c_int(0)
        _check(lib().kc_planner_explore(self.h, cell, int(r2), int(min_cost), int(min_size), C.byref(st), C.byref(comps),
                                        C.byref(kept), C.byref(passes), C.byref(lpasses)))
        return st.value, comps.value, kept.value, passes.value, lpasses.value

    def frontiers(self):
        """The kept frontiers of the last explore(), sorted by (cost, entry flat index): a structured array of
        PLAN_FRONTIER_DTYPE (sum_i, sum_j, size, root, cost, entry_i, entry_j)."""
        n = _sz(0)
        _check(lib().kc_planner_get_frontiers(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, PLAN_FRONTIER_DTYPE)
        if n.value:
            _check(lib().kc_planner_get_frontiers(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def frontier_path(self, k):
        """(n, 2) int32 cells (i, j) from the robot's cell to the entry cell of kept frontier k."""
        n = _sz(0)
        _check(lib().kc_planner_get_frontier_path(self.h, int(k), None, 0, C.byref(n)))
        cells = np.empty((n.value, 2), np.int32)
        _check(lib().kc_planner_get_frontier_path(self.h, int(k), cells.ctypes.data, n.value, C.byref(n)))
        return cells[:n.value]

    def frontier_labels(self):
        """uint32 [width, height]: the label of every frontier cell of the last explore(), PLAN_INF elsewhere."""
        w, h = self.shape
        lab = np.empty((w, h), np.uint32, order="F")
        _check(lib().kc_planner_get_frontier_labels(self.h, lab.ctypes.data, lab.size))
        return lab

    def explore_info(self):
        """(tiles labelled, all tiles, (field ms, mark + label ms, records ms)) of the last explore()."""
        listed, tiles, ms = C.c_uint32(0), C.c_uint32(0), (C.c_float * 3)()
        _check(lib().kc_planner_explore_info(self.h, C.byref(listed), C.byref(tiles), ms))
        return listed.value, tiles.value, tuple(float(v) for v in ms)


def worldmap_check_model(hit=3, miss=1, e_min=-8, e_max=14, occ_thr=1):
    """The test kc_worldmap_set_model makes of its parameters (host only); raises ValueError."""
    _check(lib().kc_worldmap_check_model(int(hit), int(miss), int(e_min), int(e_max), int(occ_thr)))


def worldmap_check_grid(world_resolution, grid_height, grid_width, central, resolution):
    """The test every world map update makes of its local grid before the device is used (host only)."""
    _check(lib().kc_worldmap_check_grid(float(np.float32(world_resolution)), int(grid_height), int(grid_width),
                                        int(central[0]), int(central[1]), float(np.float32(resolution))))


def worldmap_quantise_pose(resolution, origin, x, y, yaw) -> WorldMapPose:
    """(x, y, yaw) of a local grid's frame in a map of this resolution and origin -> WorldMapPose (host only)."""
    p = WorldMapPose()
    _check(lib().kc_worldmap_quantise_pose(float(np.float32(resolution)), float(origin[0]), float(origin[1]), float(x),
                                           float(y), float(yaw), C.byref(p)))
    return p


def worldmap_window(resolution, origin, x, y, max_sensor_range):
    """Rule 16 (host only): the centre cell and the radius in cells of the obstacle window -> (Ic, Jc, Rc)."""
    ic, jc, rc = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib().kc_worldmap_window(float(np.float32(resolution)), float(origin[0]), float(origin[1]), float(x), float(y),
                                    float(np.float32(max_sensor_range)), C.byref(ic), C.byref(jc), C.byref(rc)))
    return ic.value, jc.value, rc.value


SCAN_UNKNOWN_BLOCKS = 1  # KC_SCAN_UNKNOWN_BLOCKS


def worldmap_scan_table(angles):
    """Rule 21 (host only): int32 [n, 2] of (ac_k, as_k) = lrint(cos(a_k) 2^30), lrint(sin(a_k) 2^30)."""
    a = _f64(angles).reshape(-1)
    out = np.zeros((len(a), 2), np.int32)
    if len(a):
        _check(lib().kc_worldmap_scan_table(_pd(a), len(a), out.ctypes.data_as(_ip)))
    return out


def worldmap_scan_check(resolution, n_poses, n_beams, range_max, flags=0):
    """The refusals of rules 20, 21 and 25 (host only) -> Rc; raises ValueError / IndexError."""
    return int(_out(C.c_int32, lib().kc_worldmap_scan_check, float(np.float32(resolution)), int(n_poses), int(n_beams),
                    float(np.float32(range_max)), int(flags)))


def _scan_flags(unknown_blocks, flags):
    return int(flags) if flags is not None else (SCAN_UNKNOWN_BLOCKS if unknown_blocks else 0)


INTEGRATE_CLEAR_NO_RETURN = 1  # KC_INTEGRATE_CLEAR_NO_RETURN
INTEGRATE_MISS, INTEGRATE_HIT = 1, 2  # the bits of a mark byte (WorldMapContext.integrate_marks)


def _zq(zq):
    z = np.asarray(zq)
    if z.dtype.kind not in "iu":
        raise ValueError("quantised ranges are integers: worldmap_quantise_ranges makes them")
    if z.size and (int(z.min()) < -(1 << 31) or int(z.max()) >= (1 << 31)):
        raise ValueError("a quantised range does not fit int32")
    return np.ascontiguousarray(z, dtype=np.int32).reshape(-1)


def worldmap_integrate_check(resolution, n_beams, range_max, flags=0, zq=None):
    """Rule 52's refusals (host only) in their order: counts, range_max, flags, zq -> (Rc, ZMAX); raises ValueError /
    IndexError."""
    z = None if zq is None else _zq(zq)
    rc, zmax = C.c_int32(), C.c_int64()
    _check(lib().kc_worldmap_integrate_check(float(np.float32(resolution)), int(n_beams), float(np.float32(range_max)), int(flags),
                                             None if z is None else z.ctypes.data, C.byref(rc), C.byref(zmax)))
    return rc.value, zmax.value


def worldmap_quantise_ranges(ranges, resolution, range_max, range_min=0.0):
    """Rule 52 (host only): measured ranges in metres -> int32 [B]: -1 for a NaN, a negative range or one below range_min,
    ZMAX for +inf or a range >= range_max, else llrint(z / resolution * 65536)."""
    r = _f64(ranges).reshape(-1)
    out = np.zeros(len(r), np.int32)
    _check(lib().kc_worldmap_quantise_ranges(float(np.float32(resolution)), _pd(r), len(r), float(np.float32(range_max)),
                                             float(np.float32(range_min)), out.ctypes.data_as(_ip)))
    return out


WORLDMAP_MAX_CLUSTERS = 256  # KC_WORLDMAP_MAX_CLUSTERS


def _movers_params(m2, gap, join_q, min_beams):
    """The four as Python ints that fit the C types: a negative one is a ValueError, one too wide an IndexError (ctypes
    would wrap both silently)."""
    out = []
    for name, v, bits in (("m2", m2, 32), ("gap", gap, 32), ("join_q", join_q, 64), ("min_beams", min_beams, 32)):
        v = int(v)
        if v < 0:
            raise ValueError(f"{name} is negative")
        if v >> bits:
            raise IndexError(f"{name} does not fit {bits} bits")
        out.append(v)
    return out


def worldmap_movers_check(resolution, n_beams, range_max, zq=None, m2=4, gap=2, join_q=9 << 16, min_beams=3):
    """Rule 70's refusals (host only) in their order: rule 52's without flags, then m2, gap, join_q, min_beams -> ZMAX;
    raises ValueError / IndexError."""
    z = None if zq is None else _zq(zq)
    m2, gap, join_q, min_beams = _movers_params(m2, gap, join_q, min_beams)
    zmax = C.c_int64()
    _check(lib().kc_worldmap_movers_check(float(np.float32(resolution)), int(n_beams), float(np.float32(range_max)),
                                          None if z is None else z.ctypes.data, m2, gap, join_q, min_beams, C.byref(zmax)))
    return zmax.value


def worldmap_match_check_window(n_yaw, yaw_step, reach):
    """Rule 10's ranges of a match's window (host only); raises ValueError."""
    _check(lib().kc_worldmap_match_check_window(int(n_yaw), float(yaw_step), int(reach)))


def worldmap_match_check_grid(world_resolution, grid_height, grid_width, central, resolution):
    """The test every match makes of its local grid before the device is used (host only)."""
    _check(lib().kc_worldmap_match_check_grid(float(np.float32(world_resolution)), int(grid_height), int(grid_width),
                                              int(central[0]), int(central[1]), float(np.float32(resolution))))


def worldmap_match_rotations(yaw, n_yaw, yaw_step):
    """Rule 10's table (host only): [(Cq_k, Sq_k) for k = -n_yaw .. n_yaw]."""
    worldmap_match_check_window(n_yaw, yaw_step, 0)
    n = 2 * int(n_yaw) + 1
    rot = (WorldMapRotation * n)()
    _check(lib().kc_worldmap_match_rotations(float(yaw), int(n_yaw), float(yaw_step), rot, n))
    return [(int(r.cq), int(r.sq)) for r in rot]


def worldmap_recentre_plan(width, height, ic, jc, margin, stride):
    """Rule 49 (host only): the shift (di, dj) that recentres a width x height window on the robot's cell (ic, jc), (0, 0)
    while the cell is `margin` cells or more from every border; raises ValueError for a bad policy."""
    di, dj = C.c_int32(), C.c_int32()
    _check(lib().kc_worldmap_recentre_plan(int(width), int(height), int(ic), int(jc), int(margin), int(stride), C.byref(di),
                                           C.byref(dj)))
    return int(di.value), int(dj.value)


def worldmap_check_shift(offset, di, dj):
    """Rule 46's cap (host only): raises IndexError when a shift by (di, dj) would take `offset` above 2^30 cells."""
    _check(lib().kc_worldmap_check_shift(int(offset[0]), int(offset[1]), int(di), int(dj)))


class WorldMapContext(_Owner, _StreamOrdered):
    """Owner of one kc_worldmap context: a world-frame map on the device, fused from local grids.
    Works in cells: a plane is an array m[I, J] of (width, height) cells, I along x, as PlannerContext's grids."""
    _kc = "kc_worldmap"

    def __init__(self, width, height, resolution, origin=(0.0, 0.0), device=0):
        self.shape = (int(width), int(height))
        self.resolution = float(np.float32(resolution))
        self.origin = (float(origin[0]), float(origin[1]))
        self._open(lib().kc_worldmap_create, int(device), self.shape[0], self.shape[1], self.resolution, self.origin[0],
                   self.origin[1])

    def set_model(self, hit=3, miss=1, e_min=-8, e_max=14, occ_thr=1):
        """The update model; clears the map."""
        _check(lib().kc_worldmap_set_model(self.h, int(hit), int(miss), int(e_min), int(e_max), int(occ_thr)))

    def quantise_pose(self, x, y, yaw) -> WorldMapPose:
        return worldmap_quantise_pose(self.resolution, self.origin, x, y, yaw)

    def _pose(self, pose):
        return pose if isinstance(pose, WorldMapPose) else self.quantise_pose(*pose)

    def _grid_args(self, grid, device_ptr, shape, central, resolution):
        """-> ((pointer, grid_height, grid_width, central_i, central_j, resolution) as the C entries take a local grid, the
        array that keeps a host pointer alive).  grid: 2-D int32 on the host, any memory order; or device_ptr with shape."""
        g = None
        if device_ptr is None:
            g = np.asarray(grid)
            if g.ndim != 2 or g.dtype != np.int32:
                raise ValueError("expected a 2-D int32 grid")
            g = np.asfortranarray(g)  # local cell (i, j) at i + j * grid_height
            device_ptr, shape = g.ctypes.data, g.shape
        gh, gw = int(shape[0]), int(shape[1])
        c = (gh // 2 - 1, gw // 2 - 1) if central is None else central  # the mapper's central cell (local_mapper.h:26-27)
        res = self.resolution if resolution is None else float(np.float32(resolution))
        return (int(device_ptr), gh, gw, int(c[0]), int(c[1]), res), g

    def _update(self, entry, source, pose):
        p, r = self._pose(pose), WorldMapResult()
        _check(entry(self.h, *source, C.byref(p), C.byref(r)))
        return r.as_tuple()

    def update(self, grid, pose, central=None, resolution=None):
        """grid: int32 [grid_height, grid_width] on the host (MapperContext.scan_to_grid's form), any memory order;
        pose: (x, y, yaw) of its frame in the world, or a WorldMapPose.  -> (changed, (i_min, j_min, i_max, j_max))."""
        args, _keep = self._grid_args(grid, None, None, central, resolution)
        return self._update(lib().kc_worldmap_update_host, args, pose)

    def update_device(self, device_ptr, grid_height, grid_width, pose, central=None, resolution=None):
        """A finished int32 grid on the context's device, column-major [grid_height x grid_width], read in place."""
        args, _ = self._grid_args(None, device_ptr, (grid_height, grid_width), central, resolution)
        return self._update(lib().kc_worldmap_update_device, args, pose)

    def update_from_mapper(self, mapper: "MapperContext", pose):
        """The last grid of a MapperContext where it lies, ordered after its scan without a host wait."""
        return self._update(lib().kc_worldmap_update_from_mapper, (mapper.h,), pose)

    def _match(self, entry, source, pose, n_yaw, yaw_step, reach, rotations):
        """pose: (x, y, yaw) with n_yaw / yaw_step, or a WorldMapPose with `rotations`, the 2K + 1 (cq, sq) pairs."""
        if rotations is None:
            if isinstance(pose, WorldMapPose):
                raise ValueError("a quantised guess needs its rotation table")
            rotations = worldmap_match_rotations(pose[2], n_yaw, yaw_step)
        if len(rotations) % 2 != 1:
            raise ValueError("a rotation table holds 2 K + 1 pairs")
        rot = (WorldMapRotation * len(rotations))(*[WorldMapRotation(int(c), int(s)) for c, s in rotations])
        p, r = self._pose(pose), WorldMapMatchResult()
        _check(entry(self.h, *source, C.byref(p), rot, len(rotations) // 2, int(reach), C.byref(r)))
        return r.as_dict()

    def match(self, grid, pose, n_yaw=0, yaw_step=0.0, reach=0, central=None, resolution=None, rotations=None):
        """Rules 9 to 15: the pose of the window around the guess `pose` that puts the occupied cells of `grid` (as
        update takes it) onto the map best.  -> dict(k, u, v, score, score_guess, points, pose)."""
        args, _keep = self._grid_args(grid, None, None, central, resolution)
        return self._match(lib().kc_worldmap_match_host, args, pose, n_yaw, yaw_step, reach, rotations)

    def match_device(self, device_ptr, grid_height, grid_width, pose, n_yaw=0, yaw_step=0.0, reach=0, central=None,
                     resolution=None, rotations=None):
        """The same from a finished int32 grid on the context's device, read in place."""
        args, _ = self._grid_args(None, device_ptr, (grid_height, grid_width), central, resolution)
        return self._match(lib().kc_worldmap_match_device, args, pose, n_yaw, yaw_step, reach, rotations)

    def match_from_mapper(self, mapper: "MapperContext", pose, n_yaw=0, yaw_step=0.0, reach=0, rotations=None):
        """The same from the last grid of a MapperContext where it lies, ordered after its scan without a host wait."""
        return self._match(lib().kc_worldmap_match_from_mapper, (mapper.h,), pose, n_yaw, yaw_step, reach, rotations)

    def match_scores(self, n_yaw, reach):
        """Rule 13's table of the last match, uint32 [2K+1, 2S+1, 2S+1] indexed [k + K, v + S, u + S]; the window
        must be the one that match was given (the library checks the size)."""
        t = 2 * int(reach) + 1
        out = np.empty((2 * int(n_yaw) + 1, t, t), np.uint32)
        _check(lib().kc_worldmap_match_scores(self.h, out.ctypes.data, out.size))
        return out

    def match_set_timing(self, enable=True):
        _check(lib().kc_worldmap_match_set_timing(self.h, int(bool(enable))))

    def match_times(self):
        """(weight, points, score, pick) launches of the last match in milliseconds, by HIP events."""
        ms = (C.c_float * 4)()
        _check(lib().kc_worldmap_match_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def set_prior(self, grid):
        """grid[I, J]: an int32 or int8 (width, height) array on the host; replaces the whole state."""
        g = np.asarray(grid)
        if g.ndim != 2 or g.dtype not in (np.int32, np.int8):
            raise ValueError("expected a 2-D int32 or int8 grid")
        g = np.asfortranarray(g)
        _check(lib().kc_worldmap_set_prior_host(self.h, g.ctypes.data, g.itemsize, g.shape[0], g.shape[1]))

    def set_prior_device(self, device_ptr, width, height, elem_bytes=1):
        """A finished grid of the map's shape on the context's device (CloudContext.occupancy_grid(to_host=False):
        int8), read in place."""
        _check(lib().kc_worldmap_set_prior_device(self.h, int(device_ptr), int(elem_bytes), int(width), int(height)))

    def clear(self):
        _check(lib().kc_worldmap_clear(self.h))

    def info(self):
        """-> (width, height, resolution, (origin_x, origin_y)) as the library holds them: the origin at the current
        offset (rule 46)."""
        w, h, r, ox, oy = C.c_int(), C.c_int(), C.c_float(), C.c_double(), C.c_double()
        _check(lib().kc_worldmap_info(self.h, C.byref(w), C.byref(h), C.byref(r), C.byref(ox), C.byref(oy)))
        return w.value, h.value, r.value, (ox.value, oy.value)

    def offset(self):
        """Rule 46's (OI, OJ): the cells the window has moved since it was created."""
        oi, oj = C.c_int32(), C.c_int32()
        _check(lib().kc_worldmap_offset(self.h, C.byref(oi), C.byref(oj)))
        return int(oi.value), int(oj.value)

    def shift(self, di, dj):
        """Rule 47: move the window by whole cells, a positive di towards +x; what leaves is forgotten, what enters is
        never observed.  `origin`, which every quantisation here reads, follows (rule 46)."""
        _check(lib().kc_worldmap_shift(self.h, int(di), int(dj)))
        self.origin = self.info()[3]

    def recentre(self, x, y, margin, stride):
        """Rule 49's plan for the robot at world (x, y), then the shift -> (di, dj), the shift made."""
        di, dj = C.c_int32(), C.c_int32()
        _check(lib().kc_worldmap_recentre(self.h, float(x), float(y), int(margin), int(stride), C.byref(di), C.byref(dj)))
        self.origin = self.info()[3]  # (a refusal leaves the state, and so the origin, untouched)
        return int(di.value), int(dj.value)

    def points(self, x, y, max_sensor_range, cap=None, count_only=False):
        """Rules 16 to 19: the occupied cells within max_sensor_range of (x, y) as world-frame points, in no particular
        order -> (xyz float32 [n, 3], (i_min, i_max, j_min, j_max)), the bounds all -1 when n == 0.  count_only: ->
        (n, bounds) without the list.  cap: the points the output holds (default: as many as there are); IndexError
        when there are more."""
        n, b = _sz(0), (C.c_int32 * 4)()
        args = (self.h, float(x), float(y), float(np.float32(max_sensor_range)))
        if count_only or cap is None:
            _check(lib().kc_worldmap_points(*args, None, 0, C.byref(n), b))
            if count_only:
                return int(n.value), tuple(int(v) for v in b)
            cap = int(n.value)
        out = np.empty((int(cap), 3), np.float32)
        _check(lib().kc_worldmap_points(*args, out.ctypes.data if out.size else None, int(cap), C.byref(n), b))
        return out[:int(n.value)], tuple(int(v) for v in b)

    def scan(self, poses, angles, range_max, unknown_blocks=False, return_cells=False, flags=None):
        """Rules 20 to 27: the map's virtual laser scan.  poses: one (x, y, yaw) or WorldMapPose -> float64 [B]; a
        sequence of them -> [M, B].  return_cells: also the hit cells I + J * width, int32, -1 for no hit.  flags: the
        raw flag word instead of unknown_blocks."""
        single = isinstance(poses, WorldMapPose) or (len(poses) == 3 and np.ndim(poses[0]) == 0)
        plist = [self._pose(p) for p in ([poses] if single else poses)]
        arr = (WorldMapPose * max(len(plist), 1))(*plist)
        a = _f64(angles).reshape(-1)
        shape = (len(a),) if single else (len(plist), len(a))
        r = np.zeros(max(len(plist) * len(a), 1))
        c = np.zeros(r.size, np.int32) if return_cells else None
        _check(lib().kc_worldmap_scan(self.h, arr, len(plist), _pd(a), len(a), float(np.float32(range_max)),
                                      _scan_flags(unknown_blocks, flags), _pd(r),
                                      c.ctypes.data_as(_ip) if return_cells else None))
        n = len(plist) * len(a)
        return (r[:n].reshape(shape), c[:n].reshape(shape)) if return_cells else r[:n].reshape(shape)

    def integrate(self, pose, angles, zq, range_max, flags=0):
        """Rules 52 to 57: one measured scan into the map by an inverse ray cast.  pose: (x, y, yaw) of the scan frame or a
        WorldMapPose; angles: the beams in that frame; zq: int32 a beam as worldmap_quantise_ranges gives them; flags:
        INTEGRATE_CLEAR_NO_RETURN or 0.  -> (changed, (i_min, j_min, i_max, j_max)) as update."""
        p, r, a, z = self._pose(pose), WorldMapResult(), _f64(angles).reshape(-1), _zq(zq)
        if len(z) != len(a):
            raise ValueError("one quantised range a beam")
        _check(lib().kc_worldmap_integrate(self.h, C.byref(p), _pd(a), len(a), z.ctypes.data_as(_ip), float(np.float32(range_max)),
                                           int(flags), C.byref(r)))
        return r.as_tuple()

    def integrate_marks(self, pose, angles, zq, range_max, flags=0):
        """The mark launch of `integrate` alone -> uint8 [width, height], INTEGRATE_MISS | INTEGRATE_HIT a cell; the map is
        untouched and the mark plane zero again afterwards."""
        p, a, z = self._pose(pose), _f64(angles).reshape(-1), _zq(zq)
        if len(z) != len(a):
            raise ValueError("one quantised range a beam")
        w, h = self.shape
        out = np.zeros((w, h), np.uint8, order="F")
        _check(lib().kc_worldmap_integrate_marks(self.h, C.byref(p), _pd(a), len(a), z.ctypes.data_as(_ip),
                                                 float(np.float32(range_max)), int(flags), out.ctypes.data, out.size))
        return out

    def integrate_set_precheck(self, enable=True):
        """Measurement only: the mark kernel's byte load in front of its atomic."""
        _check(lib().kc_worldmap_integrate_set_precheck(self.h, int(bool(enable))))

    def integrate_set_timing(self, enable=True):
        _check(lib().kc_worldmap_integrate_set_timing(self.h, int(bool(enable))))

    def integrate_times(self):
        """(mark, apply) launches of the last integrate in milliseconds, by HIP events."""
        ms = (C.c_float * 2)()
        _check(lib().kc_worldmap_integrate_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def movers(self, pose, angles, zq, range_max, m2=4, gap=2, join_q=9 << 16, min_beams=3, return_labels=True):
        """Rules 64 to 69: the scan's returns that end in free space the map has seen, at least sqrt(m2) cells from
        anything occupied, grouped into runs of neighbouring beams.  pose, angles, zq as `integrate`; join_q in 2^-16
        cells^2.  The distance plane must be on (KompassHipError otherwise, and for m2 > reach^2).  The defaults are
        the prototype's values: judgement, not measurement.
        -> (labels int32 [B] or None, (n_dynamic, n_runs, n_kept, n_returned), [cluster tuples as
        WorldMapCluster.as_tuple, n_returned of them])."""
        p, a, z = self._pose(pose), _f64(angles).reshape(-1), _zq(zq)
        if len(z) != len(a):
            raise ValueError("one quantised range a beam")
        m2, gap, join_q, min_beams = _movers_params(m2, gap, join_q, min_beams)
        labels = np.zeros(max(len(a), 1), np.int32) if return_labels else None
        clusters = (WorldMapCluster * WORLDMAP_MAX_CLUSTERS)()
        rec = WorldMapMoversRecord()
        _check(lib().kc_worldmap_movers(self.h, C.byref(p), _pd(a), len(a), z.ctypes.data_as(_ip), float(np.float32(range_max)),
                                        m2, gap, join_q, min_beams, labels.ctypes.data if return_labels else None, clusters,
                                        WORLDMAP_MAX_CLUSTERS, C.byref(rec)))
        return (labels[:len(a)] if return_labels else None, rec.as_tuple(),
                [clusters[i].as_tuple() for i in range(int(rec.n_returned))])

    def movers_set_timing(self, enable=True):
        _check(lib().kc_worldmap_movers_set_timing(self.h, int(bool(enable))))

    def movers_times(self):
        """(flag, cluster) launches of the last `movers` in milliseconds, by HIP events."""
        ms = (C.c_float * 2)()
        _check(lib().kc_worldmap_movers_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def grid_device_ptr(self) -> int:
        """The cls plane on the device: int8, (width, height), what PlannerContext.set_grid_device(ptr, width, height,
        elem_bytes=1) reads in place."""
        return _out(_vp, lib().kc_worldmap_grid_device, self.h)

    def planes(self):
        """(cls int8 [width, height], evidence int8 [width, height]) copied to the host."""
        w, h = self.shape
        c = np.empty((w, h), np.int8, order="F")
        e = np.empty((w, h), np.int8, order="F")
        _check(lib().kc_worldmap_get(self.h, c.ctypes.data, e.ctypes.data, c.size))
        return c, e

    def set_distance(self, reach, unknown_blocks=False, flags=None):
        """Rules 42 and 43: keep the distance plane at `reach` cells (1 .. 254); 0 switches it off and frees it."""
        f = (WORLDMAP_DIST_UNKNOWN_BLOCKS if unknown_blocks else 0) if flags is None else int(flags)
        _check(lib().kc_worldmap_set_distance(self.h, int(reach), f))

    def distance_info(self):
        """-> (reach, flags, (i_min, j_min, i_max, j_max) the last refresh recomputed or all -1, whether that was the
        whole map)."""
        r, f, b, full = C.c_int(), C.c_uint(), (C.c_int * 4)(), C.c_int()
        _check(lib().kc_worldmap_distance_info(self.h, C.byref(r), C.byref(f), b, C.byref(full)))
        return r.value, f.value, tuple(int(v) for v in b), bool(full.value)

    def distance_refresh(self):
        _check(lib().kc_worldmap_distance_refresh(self.h))

    def distance(self):
        """dist2 uint16 [width, height] copied to the host, refreshed first; WORLDMAP_DIST_FAR beyond reach."""
        w, h = self.shape
        d = np.empty((w, h), np.uint16, order="F")
        _check(lib().kc_worldmap_get_distance(self.h, d.ctypes.data, d.size))
        return d

    def distance_device_ptr(self) -> int:
        """The refreshed plane on the device: uint16, (width, height); valid until the next set_distance."""
        return _out(_vp, lib().kc_worldmap_distance_device, self.h)


WORLDMAP_DIST_FAR = 0xFFFF  # KC_WORLDMAP_DIST_FAR
WORLDMAP_DIST_UNKNOWN_BLOCKS = 1
WORLDMAP_DIST_MAX_REACH = 254
MCL_SKIP_NO_RETURN = 2  # KC_MCL_SKIP_NO_RETURN
MCL_MODEL_NONE, MCL_MODEL_BEAM, MCL_MODEL_FIELD = 0, 1, 2
MCL_NOISE_STD = math.sqrt((65536.0 * 65536.0 - 1.0) / 3.0)  # rule 30: of the sum of four uniform 16-bit fields


def mcl_check(resolution, n_particles, n_beams, range_max, pen=None, err_shift=0, wtab=None, w_shift=0, flags=0):
    """Rule 38's refusals (host only) -> (Rc, ZMAX); raises ValueError / IndexError.  pen, wtab: None skips a table."""
    pn = None if pen is None else np.ascontiguousarray(pen, dtype=np.uint16)
    wt = None if wtab is None else np.ascontiguousarray(wtab, dtype=np.uint32)
    rc, zmax = C.c_int32(), C.c_int64()
    _check(lib().kc_mcl_check(float(np.float32(resolution)), int(n_particles), int(n_beams), float(np.float32(range_max)),
                              None if pn is None else pn.ctypes.data, 0 if pn is None else pn.size, int(err_shift),
                              None if wt is None else wt.ctypes.data, 0 if wt is None else wt.size, int(w_shift),
                              int(flags), C.byref(rc), C.byref(zmax)))
    return rc.value, zmax.value


def mcl_field_check(resolution, n_particles, n_beams, range_max, pen_d2=None, reach=0, wtab=None, w_shift=0, flags=0):
    """kc_mcl_field_check's refusals (host only) -> (Rc, ZMAX); raises ValueError / IndexError.  pen_d2, wtab: None skips a
    table; reach 0 skips the reach."""
    pn = None if pen_d2 is None else np.ascontiguousarray(pen_d2, dtype=np.uint16)
    wt = None if wtab is None else np.ascontiguousarray(wtab, dtype=np.uint32)
    rc, zmax = C.c_int32(), C.c_int64()
    _check(lib().kc_mcl_field_check(float(np.float32(resolution)), int(n_particles), int(n_beams), float(np.float32(range_max)),
                                    None if pn is None else pn.ctypes.data, 0 if pn is None else pn.size, int(reach),
                                    None if wt is None else wt.ctypes.data, 0 if wt is None else wt.size, int(w_shift),
                                    int(flags), C.byref(rc), C.byref(zmax)))
    return rc.value, zmax.value


def mcl_heading(h):
    """Rule 29 for one heading (host only) -> (Cq, Sq)."""
    cq, sq = C.c_int32(), C.c_int32()
    _check(lib().kc_mcl_heading(int(h), C.byref(cq), C.byref(sq)))
    return cq.value, sq.value


def mcl_noise_scale(sigma_units):
    """Rule 30: the int32 scale s of a sigma given in the quantity's own units (2^-16 cells, 2^-16 turns)."""
    s = round(float(sigma_units) * 65536.0 / MCL_NOISE_STD)
    if not 0 <= s <= 0x7FFFFFFF:
        raise ValueError("sigma out of range")
    return s


def mcl_quantise_ranges(ranges, resolution, range_max, flags=0):
    """Rule 33 (host): int32 [B]."""
    r, m = float(np.float32(resolution)), float(np.float32(range_max))
    zmax = round(m / r * 65536.0)
    none = -1 if int(flags) & MCL_SKIP_NO_RETURN else zmax
    return np.array([round(float(z) / r * 65536.0) if (math.isfinite(float(z)) and 0.0 <= float(z) < m) else none
                     for z in np.asarray(ranges, dtype=np.float64).reshape(-1)], np.int32)


def mcl_recovery_update(cost_sum, n, b_used, state, a_slow=4, a_fast=1, max_num=1, max_den=4):
    """Rules 60 and 61 (host only): state (slow, fast, primed) -> (state, m or -1, n_inject); raises ValueError /
    IndexError.  The defaults are the front ends': judgement, not measurement."""
    s = MclRecovery(int(state[0]), int(state[1]), int(bool(state[2])))
    m, n_inject = C.c_int64(), _sz(0)
    _check(lib().kc_mcl_recovery_update(int(cost_sum), int(n), int(b_used), int(a_slow), int(a_fast), int(max_num), int(max_den),
                                        C.byref(s), C.byref(m), C.byref(n_inject)))
    return (int(s.slow), int(s.fast), bool(s.primed)), int(m.value), int(n_inject.value)


class MclContext(_Owner):
    """Owner of one kc_mcl context (DESIGN.md 4.11 rules 28 to 41): a Monte-Carlo localiser over a WorldMapContext,
    which it keeps alive.  Works in the ABI's integers; kompass_core.mapping.MCL is the front end in metres."""
    _kc = "kc_mcl"

    def __init__(self, world_map: "WorldMapContext", n_particles, angles, range_max, seed=0):
        self.map = world_map
        a = _f64(angles).reshape(-1)
        self.n, self.n_beams = int(n_particles), len(a)
        self.range_max = float(np.float32(range_max))
        self._open(lib().kc_mcl_create, world_map.h, self.n, _pd(a), len(a), self.range_max, int(seed) & (2 ** 64 - 1))
        self.rc, self.zmax = mcl_check(world_map.resolution, self.n, self.n_beams, self.range_max)

    def set_model(self, pen, err_shift, wtab, w_shift):
        pn, wt = np.ascontiguousarray(pen, dtype=np.uint16), np.ascontiguousarray(wtab, dtype=np.uint32)
        _check(lib().kc_mcl_set_model(self.h, pn.ctypes.data, pn.size, int(err_shift), wt.ctypes.data, wt.size,
                                      int(w_shift)))

    def set_field_model(self, pen_d2, pen_far, wtab, w_shift):
        """Rules 44 and 45 in place of 32 to 34: pen_d2 has c2 + 1 entries; the map's distance plane must be on at a step."""
        pn, wt = np.ascontiguousarray(pen_d2, dtype=np.uint16), np.ascontiguousarray(wtab, dtype=np.uint32)
        if not 0 <= int(pen_far) <= 0xFFFF:
            raise ValueError("pen_far is a uint16")
        _check(lib().kc_mcl_set_field_model(self.h, pn.ctypes.data, pn.size, int(pen_far), wt.ctypes.data, wt.size, int(w_shift)))

    def model_kind(self) -> int:
        return _out(C.c_int, lib().kc_mcl_model_kind, self.h)

    def init_pose(self, tx0, ty0, h0, s_xy, s_h):
        _check(lib().kc_mcl_init_pose(self.h, int(tx0), int(ty0), int(h0), int(s_xy), int(s_h)))

    def init_global(self) -> int:
        """-> the free cells; KompassHipError (KC_ERR_STATE) when the map has none."""
        n = _sz(0)
        _check(lib().kc_mcl_init_global(self.h, C.byref(n)))
        return int(n.value)

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0) -> MclRecord:
        z = np.ascontiguousarray(zq, dtype=np.int32).reshape(-1)
        if z.size != self.n_beams:
            raise ValueError("one quantised range a beam")
        r = MclRecord()
        _check(lib().kc_mcl_step(self.h, int(d_f), int(d_l), int(d_h), int(s_f), int(s_l), int(s_h),
                                 z.ctypes.data_as(_ip), int(flags), C.byref(r)))
        return r

    def resample(self):
        _check(lib().kc_mcl_resample(self.h))

    def last_fit(self) -> MclFit:
        """Rule 59's fit of the last step, from the host copy its read-back filled; KompassHipError (KC_ERR_STATE) before
        a step and after an init or a change of model."""
        f = MclFit()
        _check(lib().kc_mcl_last_fit(self.h, C.byref(f)))
        return f

    def resample_inject(self, n_inject):
        """Rule 62: rule 40's resample with n_inject of the N slots drawn anew over the map's free cells; 0 is resample()."""
        _check(lib().kc_mcl_resample_inject(self.h, int(n_inject)))

    @staticmethod
    def recovery_update(cost_sum, n, b_used, state, a_slow=4, a_fast=1, max_num=1, max_den=4):
        """mcl_recovery_update: rules 60 and 61, host only."""
        return mcl_recovery_update(cost_sum, n, b_used, state, a_slow, a_fast, max_num, max_den)

    def inject_times(self):
        """(rows, row_prefix, inject) launches of the last injecting resample in milliseconds, by HIP events."""
        ms = (C.c_float * 3)()
        _check(lib().kc_mcl_inject_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def particles(self):
        """(tx int64, ty int64, h uint32, acc uint32), N each, copied to the host."""
        tx, ty = np.empty(self.n, np.int64), np.empty(self.n, np.int64)
        h, acc = np.empty(self.n, np.uint32), np.empty(self.n, np.uint32)
        _check(lib().kc_mcl_particles(self.h, tx.ctypes.data, ty.ctypes.data, h.ctypes.data, acc.ctypes.data, self.n))
        return tx, ty, h, acc

    def particles_device(self):
        """The four device addresses (tx, ty, h, acc): valid until the next step, resample or init."""
        p = [_vp() for _ in range(4)]
        _check(lib().kc_mcl_particles_device(self.h, *[C.byref(v) for v in p]))
        return tuple(v.value for v in p)

    def step_count(self) -> int:
        s = C.c_uint32()
        _check(lib().kc_mcl_info(self.h, None, None, None, None, C.byref(s)))
        return s.value

    def set_timing(self, enable=True):
        _check(lib().kc_mcl_set_timing(self.h, int(bool(enable))))

    def times(self):
        """(walk, weigh, prefix, select) launches in milliseconds, by HIP events; the last two 0 without a resample."""
        ms = (C.c_float * 4)()
        _check(lib().kc_mcl_times(self.h, ms))
        return tuple(float(v) for v in ms)


def _in(v, lo, hi, what):
    """int(v) when it fits the C type of the argument, ValueError otherwise (ctypes would wrap it silently)."""
    v = int(v)
    if not lo <= v <= hi:
        raise ValueError(f"{what} = {v} does not fit its C type")
    return v


def mppi_check(n_samples, horizon, n_path, limits=None, s=None, costs=None, reach=0):
    """kc_mppi_check's refusals (host only; DESIGN.md 4.12 rule 12); raises ValueError / IndexError.  limits: (F_lo, F_hi,
    L_hi, H_hi, kq) with s the three scales, or None; costs: (r2, pen_d2, pen_hit, w_path, qcap, w_goal, wtab, w_shift) or
    None."""
    lim = None if limits is None else np.array([_in(v, -2 ** 31, 2 ** 31 - 1, "limit") for v in limits], np.int32)
    sc = None if s is None else np.array([_in(v, -2 ** 31, 2 ** 31 - 1, "scale") for v in s], np.int32)
    if lim is not None and lim.size != 5 or sc is not None and sc.size != 3:
        raise ValueError("five limits and three scales")
    r2 = pen_hit = w_path = qcap = w_goal = w_shift = 0
    pn = wt = None
    if costs is not None:
        r2, pen, pen_hit, w_path, qcap, w_goal, wtab, w_shift = costs
        pn, wt = np.ascontiguousarray(pen, dtype=np.uint16), np.ascontiguousarray(wtab, dtype=np.uint32)
    u32 = 2 ** 32 - 1
    _check(lib().kc_mppi_check(int(n_samples), int(horizon), int(n_path), None if lim is None else lim.ctypes.data,
                               None if sc is None else sc.ctypes.data, _in(r2, 0, u32, "r2"),
                               None if pn is None else pn.ctypes.data, 0 if pn is None else pn.size, _in(pen_hit, 0, u32, "pen_hit"),
                               _in(w_path, 0, u32, "w_path"), _in(qcap, 0, 2 ** 64 - 1, "qcap"), _in(w_goal, 0, u32, "w_goal"),
                               int(reach), None if wt is None else wt.ctypes.data, 0 if wt is None else wt.size, int(w_shift)))


def _mover_arrays(ox, oy, vx, vy, hq, sq, g):
    """Rule 13's seven arrays in the ABI's types; a value that does not fit its C type is a ValueError, as _in has it."""
    out = []
    for a, dt, what in ((ox, np.int64, "OX"), (oy, np.int64, "OY"), (vx, np.int32, "VX"), (vy, np.int32, "VY"),
                        (hq, np.uint64, "hq"), (sq, np.uint64, "sq"), (g, np.uint64, "g")):
        info = np.iinfo(dt)
        out.append(np.array([_in(v, int(info.min), int(info.max), what) for v in np.asarray(a, dtype=object).reshape(-1)], dt))
    return out


def mppi_check_movers(ox, oy, vx, vy, hq, sq, g, pen_hit_mv, n=None):
    """kc_mppi_check_movers' refusals (host only; DESIGN.md 4.12 rule 18); raises ValueError / IndexError.  n: the count
    handed over, len(ox) by default; an array may be None (NULL)."""
    arr = [None if a is None else b for a, b in zip((ox, oy, vx, vy, hq, sq, g),
                                                    _mover_arrays(*[() if a is None else a for a in (ox, oy, vx, vy, hq, sq, g)]))]
    n = (0 if arr[0] is None else arr[0].size) if n is None else int(n)
    if any(a is not None and a.size < n for a in arr):
        raise ValueError("an array is shorter than the count")
    _check(lib().kc_mppi_check_movers(*[None if a is None else a.ctypes.data for a in arr], n, _in(pen_hit_mv, 0, 2 ** 32 - 1, "pen_hit_mv")))


def mppi_check_field(fcap, w_run, w_term):
    """kc_mppi_check_field's refusals (host only; DESIGN.md 4.12 rule 23); raises ValueError / IndexError."""
    u32 = 2 ** 32 - 1
    _check(lib().kc_mppi_check_field(_in(fcap, 0, u32, "fcap"), _in(w_run, 0, u32, "w_run"), _in(w_term, 0, u32, "w_term")))


def _i32_words(v, n, what):
    """n int32 words, or None for None; a value that does not fit its C type is a ValueError, as _in has it."""
    if v is None:
        return None
    a = np.array([_in(x, -2 ** 31, 2 ** 31 - 1, what) for x in np.asarray(v, dtype=object).reshape(-1)], np.int32)
    if a.size != n:
        raise ValueError(f"{what}: {n} words, got {a.size}")
    return a


def mppi_check_rates(rates=None, v0=None):
    """kc_mppi_check_rates' refusals (host only; DESIGN.md 4.12 rule 29); raises ValueError / IndexError.  rates: (F_up,
    F_dn, L_up, L_dn, H_up, H_dn) or None (the mode is off); v0: (F0, L0, H0) or None."""
    r, v = _i32_words(rates, 6, "rates"), _i32_words(v0, 3, "v0")
    _check(lib().kc_mppi_check_rates(None if r is None else r.ctypes.data, None if v is None else v.ctypes.data))


def mppi_apply_rates(limits, rates, v0, u):
    """kc_mppi_apply_rates (host only; rule 28): rule 26 over the sequence u, T x (F, L, H), from v0 -> int32 [T, 3].
    limits: rule 12's five words (the cone kq plays a part)."""
    lim, r, v = _i32_words(limits, 5, "limits"), _i32_words(rates, 6, "rates"), _i32_words(v0, 3, "v0")
    ui = np.array([_in(x, -2 ** 31, 2 ** 31 - 1, "u") for x in np.asarray(u, dtype=object).reshape(-1)], np.int32)
    if ui.size % 3:
        raise ValueError("the sequence is T x 3 int32")
    out = np.zeros((ui.size // 3, 3), np.int32)
    _check(lib().kc_mppi_apply_rates(*[None if a is None else a.ctypes.data for a in (lim, r, v)], ui.ctypes.data, ui.size // 3,
                                     out.ctypes.data))
    return out


def _offset_words(offsets):
    """Rule 30's offsets as int32 words, or None for None; a value that does not fit its C type is a ValueError."""
    if offsets is None:
        return None
    return np.array([_in(x, -2 ** 31, 2 ** 31 - 1, "offset") for x in np.asarray(offsets, dtype=object).reshape(-1)], np.int32)


def mppi_check_footprint(offsets=(), n=None):
    """kc_mppi_check_footprint's refusals (host only; DESIGN.md 4.12 rule 35); raises ValueError / IndexError.  offsets:
    the disc offsets in 16 fraction bits of a cell, or None (NULL); n: the count handed over, len(offsets) by default."""
    o = _offset_words(offsets)
    n = (0 if o is None else o.size) if n is None else int(n)
    if o is not None and n <= 8 and o.size < n:                            # (above 8 the library answers before it reads)
        raise ValueError("the array is shorter than the count")
    _check(lib().kc_mppi_check_footprint(None if o is None or o.size == 0 else o.ctypes.data, n))


class MppiContext(_Owner):
    """Owner of one kc_mppi context: an MPPI controller over a WorldMapContext's distance plane, which it
    keeps alive.  Works in the ABI's integers and keeps no sequence between steps; kompass_core.control.MPPI is the front
    end in metres."""
    _kc = "kc_mppi"

    def __init__(self, world_map: "WorldMapContext", n_samples, horizon, seed=0):
        self.map = world_map
        self.field_planner = None
        self.n, self.horizon = int(n_samples), int(horizon)
        self._open(lib().kc_mppi_create, world_map.h, self.n, self.horizon, int(seed) & (2 ** 64 - 1))

    def set_model(self, f_lo, f_hi, l_hi, h_hi, kq, s):
        sc = np.array([_in(v, -2 ** 31, 2 ** 31 - 1, "scale") for v in s], np.int32)
        if sc.size != 3:
            raise ValueError("three scales")
        i32 = (-2 ** 31, 2 ** 31 - 1)
        _check(lib().kc_mppi_set_model(self.h, _in(f_lo, *i32, "F_lo"), _in(f_hi, *i32, "F_hi"), _in(l_hi, *i32, "L_hi"),
                                       _in(h_hi, *i32, "H_hi"), _in(kq, *i32, "kq"), sc.ctypes.data))

    def set_costs(self, r2, pen_d2, pen_far, pen_hit, w_path, qcap, w_goal, wtab, w_shift):
        pn, wt = np.ascontiguousarray(pen_d2, dtype=np.uint16), np.ascontiguousarray(wtab, dtype=np.uint32)
        u32 = 2 ** 32 - 1
        _check(lib().kc_mppi_set_costs(self.h, _in(r2, 0, u32, "r2"), pn.ctypes.data, pn.size, _in(pen_far, 0, 0xFFFF, "pen_far"),
                                       _in(pen_hit, 0, u32, "pen_hit"), _in(w_path, 0, u32, "w_path"), _in(qcap, 0, 2 ** 64 - 1, "qcap"),
                                       _in(w_goal, 0, u32, "w_goal"), wt.ctypes.data, wt.size, int(w_shift)))

    def set_path(self, px, py):
        x, y = np.ascontiguousarray(px, dtype=np.int64).reshape(-1), np.ascontiguousarray(py, dtype=np.int64).reshape(-1)
        if x.size != y.size:
            raise ValueError("one y a x")
        _check(lib().kc_mppi_set_path(self.h, x.ctypes.data, y.ctypes.data, x.size))

    def set_movers(self, ox=(), oy=(), vx=(), vy=(), hq=(), sq=(), g=(), pen_hit_mv=0):
        """Rule 13's list for every later step, at the time of the next step's pose; none clears it."""
        arr = _mover_arrays(ox, oy, vx, vy, hq, sq, g)
        if any(a.size != arr[0].size for a in arr):
            raise ValueError("one entry a mover in every array")
        _check(lib().kc_mppi_set_movers(self.h, *[a.ctypes.data for a in arr], arr[0].size, _in(pen_hit_mv, 0, 2 ** 32 - 1, "pen_hit_mv")))

    @staticmethod
    def check_movers(ox, oy, vx, vy, hq, sq, g, pen_hit_mv, n=None):
        mppi_check_movers(ox, oy, vx, vy, hq, sq, g, pen_hit_mv, n)

    def set_field(self, planner=None, fcap=1 << 20, w_run=0, w_term=0):
        """Attaches a PlannerContext's kept cost field (rules 19 to 24) for every later step, and keeps the planner alive;
        None detaches and returns to the path mode."""
        if planner is None:
            _check(lib().kc_mppi_set_field(self.h, None, 0, 0, 0))
            self.field_planner = None
            return
        u32 = 2 ** 32 - 1
        _check(lib().kc_mppi_set_field(self.h, planner.h, _in(fcap, 0, u32, "fcap"), _in(w_run, 0, u32, "w_run"),
                                       _in(w_term, 0, u32, "w_term")))
        self.field_planner = planner

    def last_field(self):
        """(f0, f_nom) of the last step (rule 22): the uncapped field value of the pose's cell, 0xFFFFFFFF in an invalid or
        cut-off cell or outside the map, and the nominal sample's fl."""
        f0, fn = C.c_uint32(0), C.c_uint32(0)
        _check(lib().kc_mppi_last_field(self.h, C.byref(f0), C.byref(fn)))
        return f0.value, fn.value

    def set_rates(self, rates=None):
        """Rule 25's six rates (F_up, F_dn, L_up, L_dn, H_up, H_dn) for every later step: every sample is rolled out by
        its applied control (rules 26 and 27).  None turns the mode off."""
        r = _i32_words(rates, 6, "rates")
        _check(lib().kc_mppi_set_rates(self.h, None if r is None else r.ctypes.data))

    def set_velocity(self, v0):
        """Rule 25's V0 = (F0, L0, H0), the robot's velocity in front of the next step, until the next call; zero in a
        new context.  It plays a part only while rates are set."""
        v = _i32_words(v0, 3, "v0")
        _check(lib().kc_mppi_set_velocity(self.h, None if v is None else v.ctypes.data))

    def set_footprint(self, offsets=()):
        """Rule 30's disc offsets along the body's forward axis (16 fraction bits of a cell, at most 8) for every later
        step: rule 5 runs on the least plane value under the discs (rules 31 and 32).  None clear the list."""
        o = _offset_words(() if offsets is None else offsets)
        _check(lib().kc_mppi_set_footprint(self.h, o.ctypes.data if o.size else None, o.size))

    def step(self, tx, ty, h, u, step):
        """-> (U' int32 [T, 3], MppiRecord).  u: the nominal sequence, T x (F, L, H)."""
        ui = np.ascontiguousarray(u, dtype=np.int64).reshape(-1)
        if ui.size != 3 * self.horizon or ui.size and (ui.min() < -2 ** 31 or ui.max() > 2 ** 31 - 1):
            raise ValueError("the sequence is T x 3 int32")
        ui = ui.astype(np.int32)
        out, r = np.zeros((self.horizon, 3), np.int32), MppiRecord()
        _check(lib().kc_mppi_step(self.h, _in(tx, -2 ** 63, 2 ** 63 - 1, "tx"), _in(ty, -2 ** 63, 2 ** 63 - 1, "ty"),
                                  _in(h, 0, 2 ** 32 - 1, "h"), ui.ctypes.data, _in(step, 0, 2 ** 32 - 1, "step"), out.ctypes.data,
                                  C.byref(r)))
        return out, r

    def costs(self):
        """All S_k of the last step: uint32 [K]."""
        s = np.empty(self.n, np.uint32)
        _check(lib().kc_mppi_costs(self.h, s.ctypes.data, self.n))
        return s

    def set_team(self, lanes):
        """Measurement only: 1, 4 or 8 lanes a sample in the roll-out; no result depends on it."""
        _check(lib().kc_mppi_set_team(self.h, int(lanes)))

    def set_timing(self, enable=True):
        _check(lib().kc_mppi_set_timing(self.h, int(bool(enable))))

    def times(self):
        """(rollout, update) launches of the last step in milliseconds, by HIP events."""
        ms = (C.c_float * 2)()
        _check(lib().kc_mppi_times(self.h, ms))
        return tuple(float(v) for v in ms)
