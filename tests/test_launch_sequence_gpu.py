"""The launch sequence of the DWA host path, option by option: the names timings() returns for one sensor update, one
cycle, then rollout + evaluate on the smallest DWA context (test_context_lifecycle.make_dwa: 16 samples, 8 poses,
64 points), and the result of both -- found, cost, index, the winner's rows -- bit for bit.

The host path decides every launch in a plan (csrc/kc_launch_plan.h) and then carries it out; the decisions themselves
are tested without a GPU (tests/test_launch_plan_cpu.py).  This file pins what reaches the stream."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
import test_context_lifecycle as lifecycle  # noqa: E402

INP = lifecycle._dwa_inputs()
ANGLES16, RANGES16 = syn.dense_scan(16, 0.2)
# the dropped-cycle case: the smallest straight segment with which the 16-sample lattice's cycle tables stop fitting
# beside the roll-out tile -- found on the commit before this one by watching cycle_kernel give way to
# rollout_collide_kernel (S - 1 still takes the single launch: the second dropped case below)
DROP_S = 8961
TILT = (float(np.sin(0.15)), 0.0, 0.0, float(np.cos(0.15)))  # the sensor mount rolled by 0.3 rad

# name -> (options, sensor, context overrides)
CASES = {
    "points": ({}, "points", {}),
    "scan16": ({}, "scan", {}),
    "sensor_two_launch": ({"sensor_two_launch": 1}, "points", {}),
    "sensor_on_host": ({"sensor_on_host": 1}, "points", {}),
    "unfused_block": ({"fused_cycle": 0, "cost_kernel": 1}, "points", {}),
    "unfused_wave": ({"fused_cycle": 0, "cost_kernel": 2}, "points", {}),
    "cost_batch_forced": ({"fused_cycle": 0, "cost_kernel": 2, "cost_batch": 2}, "points", {}),
    "force_split": ({"force_split": 1}, "points", {}),
    "force_split_keep": ({"force_split": 1, "drop_samples": 0}, "points", {}),
    "host_trig": ({"device_trig": 0}, "points", {}),
    "sphere": ({}, "points", {"shape": kh.SPHERE, "dims": [0.3]}),
    "tilted": ({}, "scan", {"rot": TILT}),  # (a LaserScan: what tilts the octree frame)
    "empty_shard": ({}, "points", {"shard": (0, 0)}),
    "cycle_kept": ({}, "points", {"S": DROP_S - 1}),
    "cycle_dropped": ({}, "points", {"S": DROP_S}),
}


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def _result(ctx, r):
    out = [int(r.found), np.float32(r.cost).tobytes().hex(), int(r.index), int(r.raw_index), int(r.n_admissible)]
    if r.found:
        px, py, v = ctx.get_best()
        out.append(_digest(px, py, *v))
    return out


def run_case(name):
    """-> [names after the sensor update, names after the cycle, names after rollout + evaluate + fetch],
    [result of the cycle, result of rollout + evaluate]"""
    opts, sensor, over = CASES[name]
    rb = INP["robot"]
    S = over.get("S", len(INP["seg_xyz"]))
    seg, acc = (INP["seg_xyz"], INP["acc_at_seg"]) if "S" not in over else syn.straight_segment(S)[:2]
    ctx = kh.DwaContext(over.get("shape", rb["shape"]), over.get("dims", rb["dims"]), (0, 0, 0), over.get("rot", (0, 0, 0, 1)),
                        INP["octree_res"], INP["dt"], max_samples=64, max_points=INP["P"], max_segment=S,
                        max_obstacles=64, acc_limits=INP["acc_limits"])
    with ctx:
        ctx.timing_enable(True)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_weights(kh.make_weights(*INP["weights"]))
        ctx.set_samples(INP["vx"], INP["vy"], INP["omega"])
        if "shard" in over:
            ctx.set_shard(*over["shard"])
        ctx.set_tracked_segment(seg, acc, INP["ref_len"])
        if sensor == "scan":
            ctx.set_scan(INP["state"], RANGES16, ANGLES16, INP["max_range"])
        else:
            ctx.set_points(INP["state"], INP["points"], INP["max_range"])
        names = [[n for n, _ in ctx.timings()]]
        r = ctx.cycle(INP["state"], INP["P"])
        names.append([n for n, _ in ctx.timings()])
        results = [_result(ctx, r)]
        ctx.rollout(INP["state"], INP["P"])
        ctx.evaluate()
        r = ctx.fetch_result()
        names.append([n for n, _ in ctx.timings()])
        results.append(_result(ctx, r))
    return names, results


# What run_case returned at the commit before this one: recorded from a run of that commit's library on an MI355X
# (loaded through KOMPASS_HIP_LIB), never from the code under test.
PARENT = {'cost_batch_forced': ([['sensor_fused_kernel'],
                        ['rollout_collide_kernel', 'segment_near_kernel', 'sample_cost_batched_kernel', 'host:launch_rollout',
                         'host:launch_collision', 'host:launch_evaluate', 'host:wait_result'],
                        ['rollout_collide_kernel', 'sample_cost_batched_kernel', 'host:launch_rollout', 'host:launch_collision',
                         'host:launch_evaluate', 'host:wait_result']],
                       [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'cycle_dropped': ([['sensor_fused_kernel'],
                    ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
                     'host:wait_result'],
                    ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
                     'host:wait_result']],
                   [[1, 'fe9fba3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, 'fe9fba3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'cycle_kept': ([['sensor_fused_kernel'], ['segment_near_kernel', 'cycle_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
                 ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
                  'host:wait_result']],
                [[1, 'fc9fba3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, 'fc9fba3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'empty_shard': ([['sensor_fused_kernel'], ['host:launch_evaluate', 'host:wait_result'], ['host:launch_evaluate', 'host:wait_result']],
                 [[0, '00000000', -1, -1, 0], [0, '00000000', -1, -1, 0]]),
 'force_split': ([['sensor_fused_kernel'],
                  ['segment_near_kernel', 'trig_table_kernel', 'rollout_kernel', 'compact_kernel', 'sample_cost_kernel', 'host:launch_rollout',
                   'host:window_bits', 'host:launch_collision', 'host:launch_evaluate', 'host:wait_result'],
                  ['trig_table_kernel', 'rollout_kernel', 'compact_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:window_bits',
                   'host:launch_collision', 'host:launch_evaluate', 'host:wait_result']],
                 [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'force_split_keep': ([['sensor_fused_kernel'],
                       ['segment_near_kernel', 'trig_table_kernel', 'rollout_kernel', 'compact_kernel', 'sample_cost_kernel', 'host:launch_rollout',
                        'host:window_bits', 'host:launch_collision', 'host:launch_evaluate', 'host:wait_result'],
                       ['trig_table_kernel', 'rollout_kernel', 'compact_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:window_bits',
                        'host:launch_collision', 'host:launch_evaluate', 'host:wait_result']],
                      [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'host_trig': ([['sensor_fused_kernel'],
                ['segment_near_kernel', 'cycle_kernel', 'host:trig_table', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
                ['rollout_collide_kernel', 'sample_cost_kernel', 'host:trig_table', 'host:launch_rollout', 'host:launch_collision',
                 'host:launch_evaluate', 'host:wait_result']],
               [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'points': ([['sensor_fused_kernel'], ['segment_near_kernel', 'cycle_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
             ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
              'host:wait_result']],
            [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'scan16': ([['sensor_fused_kernel'], ['segment_near_kernel', 'cycle_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
             ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
              'host:wait_result']],
            [[1, '26e61040', 15, 15, 16, '51144eb02cc778b9'], [1, '26e61040', 15, 15, 16, '51144eb02cc778b9']]),
 'sensor_on_host': ([['dilate_kernel'], ['segment_near_kernel', 'cycle_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
                     ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
                      'host:wait_result']],
                    [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'sensor_two_launch': ([['sensor_points_kernel', 'sensor_place_kernel', 'dilate_kernel'],
                        ['segment_near_kernel', 'cycle_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
                        ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
                         'host:wait_result']],
                       [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'sphere': ([['sensor_fused_kernel'], ['segment_near_kernel', 'cycle_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:wait_result'],
             ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
              'host:wait_result']],
            [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'tilted': ([['dilate_kernel'],
             ['segment_near_kernel', 'trig_table_kernel', 'rollout_kernel', 'collision_tilted_kernel', 'compact_kernel', 'sample_cost_kernel',
              'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate', 'host:wait_result'],
             ['trig_table_kernel', 'rollout_kernel', 'collision_tilted_kernel', 'compact_kernel', 'sample_cost_kernel', 'host:launch_rollout',
              'host:launch_collision', 'host:launch_evaluate', 'host:wait_result']],
            [[1, '0c171140', 15, 15, 16, '51144eb02cc778b9'], [1, '0c171140', 15, 15, 16, '51144eb02cc778b9']]),
 'unfused_block': ([['sensor_fused_kernel'],
                    ['rollout_collide_kernel', 'sample_cost_block_kernel', 'publish_kernel', 'host:launch_rollout', 'host:launch_collision',
                     'host:launch_evaluate', 'host:wait_result'],
                    ['rollout_collide_kernel', 'sample_cost_block_kernel', 'publish_kernel', 'host:launch_rollout', 'host:launch_collision',
                     'host:launch_evaluate', 'host:wait_result']],
                   [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']]),
 'unfused_wave': ([['sensor_fused_kernel'],
                   ['rollout_collide_kernel', 'segment_near_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision',
                    'host:launch_evaluate', 'host:wait_result'],
                   ['rollout_collide_kernel', 'sample_cost_kernel', 'host:launch_rollout', 'host:launch_collision', 'host:launch_evaluate',
                    'host:wait_result']],
                  [[1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c'], [1, '174cab3f', 11, 11, 16, 'b58955671fd9ad7c']])}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_and_result_are_the_parents(name):
    names, results = run_case(name)
    want_names, want_results = PARENT[name]
    assert names == want_names
    assert results == want_results


def test_the_dropped_cycle_case_drops_the_cycle():
    # (what the two segment lengths are for: one launch at DROP_S - 1, the plain roll-out shape at DROP_S)
    assert "cycle_kernel" in PARENT["cycle_kept"][0][1]
    assert "cycle_kernel" not in PARENT["cycle_dropped"][0][1]
    assert "rollout_collide_kernel" in PARENT["cycle_dropped"][0][1]
