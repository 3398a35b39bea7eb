"""The fp16 library build (libdat_hip_f16.so: the same sources with -DDAT_H16_IS_FP16, cfg.HIP.DTYPE 'fp16'), kernel by kernel.

The 16-bit format belongs to the loaded library, so the format-generic kernel tests run again in ONE child process started with
DAT_H16=fp16: tests/test_gpu_kernels.py, tests/test_gpu_fp16_edges.py, tests/test_gpu_infer_kernels.py, tests/test_gpu_wgrad.py (the
weight-gradient kernels), tests/test_gpu_temporal_windows.py (the conv frame windows), tests/test_gpu_weight_pack.py and tests/test_gpu_dgrad.py (the weight
packers and the dense data gradient), tests/test_gpu_proposals.py (proposal selection, collect and the detection limit at their tie edges),
tests/test_gpu_batch_invariance.py (an image's head results do not depend on its batch) and the persistent-kernel test of tests/test_gpu_model.py.
The parent reads the child's JUnit report: no failure or error, every skip is a bf16-only test, and one test per kernel family (plus
the NMS and proposal goldens) is among the passed -- so that a collection mistake cannot pass for a green run.  The child is never
retried."""
import os
import subprocess
import sys
import time
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_FILES = ['tests/test_gpu_kernels.py', 'tests/test_gpu_fp16_edges.py', 'tests/test_gpu_infer_kernels.py', 'tests/test_gpu_wgrad.py',
               'tests/test_gpu_temporal_windows.py', 'tests/test_gpu_weight_pack.py', 'tests/test_gpu_dgrad.py', 'tests/test_gpu_proposals.py',
               'tests/test_gpu_model.py::test_persistent_kernel_cu_share_does_not_change_results', 'tests/test_gpu_batch_invariance.py']

K = 'tests.test_gpu_kernels::'
E = 'tests.test_gpu_fp16_edges::'
I = 'tests.test_gpu_infer_kernels::'
G = 'tests.test_gpu_wgrad::'
W = 'tests.test_gpu_temporal_windows::'
P = 'tests.test_gpu_weight_pack::'
D = 'tests.test_gpu_dgrad::'
R = 'tests.test_gpu_proposals::'
B = 'tests.test_gpu_batch_invariance::'
MUST_PASS = [
    K + 'test_layout_roundtrip[1]',
    K + 'test_conv3d[3x3x3-bf16]',                                   # generic kernel + the split-K finish
    K + 'test_conv3d[heads_100x14x14_c512-bf16]',
    K + 'test_conv3x3_c64_weights_stationary[res2_like]',           # ws64
    K + 'test_conv1x1_k64_c256_weights_stationary[many_tiles]',     # 256-channel pointwise
    K + 'test_conv3x3_linear_tiles_100_maps_512_channels',
    K + 'test_conv3x3x3_linear_strips_per_frame[2x4x24x42_128_256-bp128_ks3]',
    K + 'test_conv3x3x3_linear_strips_with_key_frame_outputs',
    K + 'test_conv3x3_big_tile[3x3x3_ragged_16x16]',
    K + 'test_conv_block_order_switch_is_bit_identical[split_k_4_cout_blocks]',
    K + 'test_conv3d_large_pointwise_layers[group4_k256_sum-bf16]',
    K + 'test_conv1x1_weights_in_lds_kernel[k128_c512_sum]',        # lw
    K + 'test_conv1x1_k_streaming_kernel[k1024_c256_mask]',         # ks
    K + 'test_stem_conv1[1]',
    K + 'test_fused_stem_conv_matches_torch[bf16]',
    K + 'test_fused_stem_and_maxpool_at_bench_size',
    K + 'test_stem_conv_pool_fused_equals_two_kernels[False-shape1-bf16]',
    K + 'test_stem_from_uint8_frames_is_bit_identical_to_the_blob_path[720-1280-800-1333-2-32-bf16]',
    K + 'test_maxpool[1]',
    K + 'test_roi_align_single_level[1]',
    K + 'test_kps_tail[1]',
    K + 'test_conv_one_pixel_wide_tiles[bf16]',
    K + 'test_full_size_layers_spot_checked[4]',
    K + 'test_batched_proposals_collect_and_box_results_equal_the_one_image_calls[1]',
    K + 'test_device_preprocessing_is_bit_identical_to_the_host_path[720-1280-800-1333-1-32]',
    K + 'test_nms_boxes_bit_exact_vs_reference[nms_n1000_t7]',
    K + 'test_nms_beyond_4096_boxes_bit_exact_vs_reference_cython[12000]',
    K + 'test_rpn_proposals_vs_reference_golden[gp_fpn3]',
    K + 'test_box_results_on_device_match_the_real_reference[pp_boxes_k5]',
    K + 'test_heatmaps_to_keypoints_matches_the_oracle[1-0-56-9]',
    E + 'test_sums_beyond_the_half_range_brought_back_by_the_affine_scale[splitk_3x3x3]',
    E + 'test_outputs_beyond_the_range_saturate_with_round_to_nearest_even[ks_1x1]',
    E + 'test_subnormal_operands_and_outputs[big_tile_3x3]',
    E + 'test_layout_conversion_is_torch_rounding_bit_for_bit',
    'tests.test_gpu_model::test_persistent_kernel_cu_share_does_not_change_results',
    I + 'test_roi_align[tube3_adaptive_c72-16]',                      # four FPN levels, tube rois, 16-bit maps
    I + 'test_roi_align[two_grid_passes_c256-16]',
    I + 'test_kps_finalize_tile_kernel[4-2-28-128-16]',
    I + 'test_time_avg[3-3-5x7x13-16]',
    I + 'test_copy_frames[4012-129]',
    G + 'test_wgrad_dma9_kernel_sub2_and_sub1_every_split[130to70_k333_s1_n1t2_7x7]',
    G + 'test_wgrad_pw_kernel_8_and_10_panels_every_tile_and_split[256to128_k111_s2_n1t2_6x2]',
    G + 'test_wgrad_pw_kernel_grouped_launch_against_the_reference',
    G + 'test_wgrad_direct_kernel_temporal_and_stride2_layers[230to128_k311_s1_n1t4_6x7]',
    G + 'test_wgrad_direct_kernel_temporal_and_stride2_layers[230to128_k311_s1_n1t8_16x17]',       # several K ranges
    G + 'test_cq_pack_and_wgrad_gemm_kernel_f32_on_every_geometry[64to128_k333_s2_n1t3_9x11]',
    G + 'test_cq_pack_and_wgrad_gemm_kernel_bf16_under_direct_0[64to128_k333_s2_n1t4_9x11_win2+2]',
    G + 'test_wgrad_finish_batch_kernel_transposes_scales_and_accumulates[0]',
    G + 'test_results_on_maps_wider_than_one_column_are_bit_identical_to_the_recorded_ones',
    W + 'test_short_clips[short_t1-outall-inall-affine_res_relu]',              # generic kernel, a split-K slice with an empty patch range
    W + 'test_temporal_k311_windows[k311-outall-in1+2-affine_res_relu]',        # windowed kT x 1 x 1: the one-tap variant
    W + 'test_big_tile_windows[big_tile-outall-in1+1-none]',                    # big-tile kernel, a frame without a valid tap
    P + 'test_per_layer_packer_is_bit_equal_to_the_expected_image[72x130x3x3x3-dgrad-16]',   # data-gradient packer, ragged, fp16 rounding
    P + 'test_batched_packer_is_bit_equal_to_the_expected_images[16]',
    D + 'test_generic_64_wide_table_driven[k333_same-16]',                     # data gradient: generic 3 x 3 x 3 ...
    D + 'test_generic_64_wide_table_driven[k333_pad_t0-16]',                   # ... and with the T padding 2
    D + 'test_k_streaming_1x1',
    D + 'test_zero_insertion_3x3x3_stride2[k333_s2_13x16]',
    D + 'test_weights_in_lds_1x1',
    R + 'test_16_bit_head',                                                     # proposals from a 16-bit head: equal keys, exact order
    B + 'test_rows_of_an_image_in_a_batched_launch_equal_the_launch_alone[kps_conv3x3_512-20-2-h16]',   # per-RoI layers planned for one image's rows
    B + 'test_rows_of_an_image_in_a_batched_launch_equal_the_launch_alone[fc6-300-4-h16]',               # ... with the rows on W
    B + 'test_table_can_fail[deconv_subpixel]',
    B + 'test_heads_on_one_image_of_a_batch_equal_the_heads_alone[r18_fpn3d-4-h16]',                      # the heads as the executor runs them, fp16 blobs
    B + 'test_a_clip_does_not_depend_on_its_companion_or_its_slot[c4_tube_gn]',
]


def test_fp16_build_passes_the_kernel_suite(tmp_path):
    xml = str(tmp_path / 'fp16_suite.xml')
    env = dict(os.environ, DAT_H16='fp16', PYTHONPATH=REPO)
    env.pop('DAT_LIB', None)
    cmd = [sys.executable, '-m', 'pytest', '-m', 'gpu', '-q', '-p', 'no:cacheprovider', '--junitxml=' + xml] + CHILD_FILES
    t0 = time.time()
    try:
        p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    except subprocess.TimeoutExpired as e:
        out = (e.output or b'').decode(errors='replace')
        pytest.fail('the fp16 child run did not finish in 1200 s:\n' + out[-4000:])
    secs = time.time() - t0
    out = p.stdout.decode(errors='replace')
    assert os.path.exists(xml), 'the fp16 child wrote no report (exit %d):\n%s' % (p.returncode, out[-4000:])
    passed, skipped, failed = [], [], []
    for case in ET.parse(xml).getroot().iter('testcase'):
        tid = case.get('classname') + '::' + case.get('name')
        bad = [c for c in case if c.tag in ('failure', 'error')]
        skip = [c for c in case if c.tag == 'skipped']
        if bad:
            failed.append('%s: %s' % (tid, (bad[0].get('message') or '')[:300]))
        elif skip:
            skipped.append((tid, skip[0].get('message') or ''))
        else:
            passed.append(tid)
    print('fp16 child: %d passed, %d skipped, %d failed in %.0f s (exit %d)' % (len(passed), len(skipped), len(failed), secs, p.returncode))
    assert not failed, 'fp16 build failures:\n' + '\n'.join(failed) + '\n' + out[-3000:]
    assert p.returncode == 0, out[-4000:]
    # (besides the bf16-only tests, only the one skip that does not depend on the build: the compiled reference op is absent in
    # both processes alike when oracle/_ref was never built)
    wrong_skips = [(t, m) for t, m in skipped if 'bf16 build only' not in m and 'oracle/_ref/libref_affine.so was never built' not in m]
    assert not wrong_skips, 'skips in the fp16 build that are not bf16-only tests: %r' % wrong_skips[:10]
    missing = [t for t in MUST_PASS if t not in set(passed)]
    assert not missing, 'must-pass tests that did not pass in the fp16 build: %r' % missing
