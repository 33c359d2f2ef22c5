"""The C-ABI library builds, loads without a GPU and exports every symbol include/dmh_hip.h declares."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(REPO, "include", "dmh_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dmh_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from depthmodelhardening_amd import _native
    from depthmodelhardening_amd.build import build
    build(verbose=False)
    lib = _native.lib()
    names = _declared()
    assert len(names) >= 23
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_native.EXPORTS) == names, "ctypes signature table and header disagree"
    assert b"gfx950" in lib.dmh_version()


def test_struct_layouts_match_the_header(tmp_path):
    from depthmodelhardening_amd import _native
    src = tmp_path / "sz.c"
    src.write_text('#include "dmh_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(dmh_photo_args),sizeof(dmh_smooth_args),sizeof(dmh_paste_args),'
                   'offsetof(dmh_photo_args,seed),offsetof(dmh_paste_args,mode),sizeof(dmh_roi_glue_args),'
                   'offsetof(dmh_roi_glue_args,B),offsetof(dmh_roi_glue_args,elu));return 0;}\n')
    exe = tmp_path / "sz"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(REPO, "include"), src, exe)) == 0
    out = os.popen(str(exe)).read().split()
    assert [int(v) for v in out] == [ctypes.sizeof(_native.PhotoArgs), ctypes.sizeof(_native.SmoothArgs),
                                     ctypes.sizeof(_native.PasteArgs), _native.PhotoArgs.seed.offset,
                                     _native.PasteArgs.mode.offset, ctypes.sizeof(_native.RoiGlueArgs),
                                     _native.RoiGlueArgs.B.offset, _native.RoiGlueArgs.elu.offset]


def test_host_side_argument_checks_without_gpu():
    """Shape errors are rejected on the host before any launch (no GPU needed)."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    a = N.PasteArgs()
    assert lib.dmh_eot_paste_fwd(ctypes.byref(a), None, None, None) == 1
    assert b"null input" in lib.dmh_last_error() or b"requirement" in lib.dmh_last_error()
    assert lib.dmh_pgd_linf_step(None, None, None, 0.1, 0.1, None, 0, None) == 1
    p = N.PhotoArgs()
    assert lib.dmh_photo_loss_fwd(ctypes.byref(p), (ctypes.c_void_p * 4)(), (ctypes.c_void_p * 4)(), None, None) == 1


def test_launch_forms_of_the_eot_paste_without_gpu():
    """K3's forward switches kernel by output width, pointer alignment and resize ratio; dmh_eot_paste_fwd decides through
    dmh_eot_paste_fwd_form, and tests/test_gpu_paste_anchor.py asserts through it which form each of its cases reached.
    The workload's forms (2 = tiled, 1 = four-wide, 0 = generic): a change of RMAX / CMAX shows here."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    one, off = ctypes.c_void_p(64), ctypes.c_void_p(68)      # dummies: 16-byte aligned, and one float off
    a = N.PasteArgs()
    assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, one) == -1
    a.scene, a.patch, a.pmask, a.coeffs = one, one, one, one
    a.N, a.SH, a.SW, a.PH, a.PW, a.l_pad, a.t_pad = 12, 375, 1242, 260, 300, 471, 57
    for (OH, OW), form in (((320, 1024), 2), ((330, 1100), 2), ((288, 960), 1), ((375, 1242), 0), ((192, 640), 1)):
        a.OH, a.OW = OH, OW
        assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, one) == form, (OH, OW)
        assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, None) == form and lib.dmh_eot_paste_fwd_form(ctypes.byref(a), None, one) == form
    a.OH, a.OW = 320, 1024
    assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), off, one) == 0 and lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, off) == 0
    assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), None, None) == -1 and b"no output" in lib.dmh_last_error()
    a.mode = N.PASTE_WARP_ONLY
    a.scene = None
    assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, one) == 2
    a.mode = N.PASTE_COMPOSITE
    assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, one) == -1          # a composite needs its scene
    a.mode = 7
    assert lib.dmh_eot_paste_fwd_form(ctypes.byref(a), one, one) == -1


def test_convolution_entry_points_reject_bad_shapes_without_gpu():
    """K10-K13 / K9 statistics: host-side argument checks and size helpers (no launch, no GPU)."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)           # a non-NULL dummy: every call below must fail before any launch
    assert lib.dmh_wino_weight_size(64, 64) == (64 // 8) * 16 * 2 * 64 * 4
    assert lib.dmh_wino_weight_size(96, 32) == (32 // 8) * 16 * 2 * 128 * 4      # output channels padded to 64s
    assert lib.dmh_wino_weight_size(64, 12) == -1
    assert lib.dmh_wino32_weight_size(32, 96) == (96 // 8) * 16 * 2 * 32 * 4
    assert lib.dmh_wino32_weight_size(96, 32) == (32 // 8) * 16 * 2 * 96 * 4       # output channels padded to 32s
    assert lib.dmh_wino32_conv3x3(one, one, None, 1, 16, 32, 8, 8, 1, one, None) != 0        # < 24 input channels
    assert lib.dmh_wino_wrw_workspace_size(2, 64, 64, 16, 32, 1) > 0 and lib.dmh_wino_wrw_workspace_size(2, 96, 32, 16, 32, 1) > 0 and lib.dmh_wino_wrw_workspace_size(2, 48, 64, 16, 32, 1) == -1 and lib.dmh_wino_wrw_workspace_size(2, 64, 64, 16, 24, 1) == -1
    assert lib.dmh_wino_wrw(one, one, 1, 64, 48, 8, 8, 1, one, one, None) != 0                # K not a multiple of 32
    assert lib.dmh_wino_conv3x3(one, one, None, 1, 16, 64, 8, 8, 1, one, None) != 0          # < 24 input channels
    assert b"multiple of 8" in lib.dmh_last_error()
    assert lib.dmh_wino_conv3x3(one, one, None, 1, 32, 64, 9, 8, 1, one, None) != 0          # odd output height
    assert lib.dmh_wino_conv3x3_act(one, one, None, None, 1, 1, 32, 64, 8, 8, 3, one, None) != 0   # pad
    # the workspace forms check their shapes before anything else (a NULL workspace is legal: whole items)
    assert lib.dmh_wino_conv3x3_ws(one, one, None, 1, 16, 64, 8, 8, 1, one, None, 0, None) != 0
    assert lib.dmh_wino_conv3x3_ws(one, one, None, 1, 32, 64, 9, 8, 1, one, one, 1 << 23, None) != 0
    assert lib.dmh_wino_conv3x3_act_ws(one, one, None, None, 1, 1, 32, 64, 8, 8, 3, one, one, 1 << 23, None) != 0
    assert lib.dmh_wino32_conv3x3_ws(one, one, None, 1, 16, 32, 8, 8, 1, one, one, 1 << 23, None) != 0
    assert lib.dmh_avg_pyramid(one, 3, 321, 1024, one, one, one, None) != 0                 # sizes must be multiples of 8
    # K15's image form: sizes, and the 16-byte alignment the wide loaders need
    assert lib.dmh_down_conv_image_size(128, 64) == (128 // 32) * (64 // 8) * 2560
    assert lib.dmh_down_conv_image_size(48, 64) == -1 and lib.dmh_down_conv_image_size(64, 12) == -1
    assert lib.dmh_down_conv_weight_image(one, None, 48, 64, one, None) != 0
    assert lib.dmh_down_conv_fwd_img(one, one, 1, None, None, 0, 1, 64, 128, 8, 10, one, one, None) != 0      # W % 4
    assert b"multiple of 4" in lib.dmh_last_error()
    assert lib.dmh_down_conv_fwd_img(one, one, 1, None, None, 0, 1, 64, 128, 8, 8, one, None, None) != 0       # yd missing
    assert lib.dmh_down_conv_bwd_data_img(one, one, one, None, 1, 64, 128, 8, 12, one, None) != 0              # W % 8
    assert lib.dmh_down_conv_bwd_data_img(one, one, one, None, 1, 48, 128, 8, 16, one, None) != 0              # C_in % 64
    assert lib.dmh_gt_depth_mse_fwd(one, one, one, 0, one, 0, 64, 0.1, 100.0, one, one, None) != 0   # empty batch
    assert lib.dmh_conv3x3_small(one, one, None, 1, 64, 64, 8, 8, 1, 0, one, None) != 0
    assert b"channel counts" in lib.dmh_last_error()
    assert lib.dmh_conv3x3_head(one, one, None, 1, 24, 8, 8, 1, one, None) != 0
    assert lib.dmh_conv7x7s2_bwd_data(one, one, 1, 64, 5, 8, 8, one, None) != 0               # > 4 image channels
    assert lib.dmh_conv7x7s2_bwd_data(one, one, 1, 64, 3, 7, 8, one, None) != 0               # odd height
    assert lib.dmh_bn_stats_partials_size(2, 8, 100) == 8 * 1 * 3
    assert lib.dmh_bn_stats_partials_size(32, 64, 160 * 512) == 64 * 64 * 3
    assert lib.dmh_bn_stats_partials_size(0, 8, 100) == -1
    assert lib.dmh_stem_bn_relu_pool_fwd(one, one, one, 1, 2, 3, 4, one, one, one, None) != 0
    assert b"even" in lib.dmh_last_error()


def test_window_entry_points_reject_bad_shapes_without_gpu():
    """K19 (windowed glue / cost / encoder-head passes) and the stand-alone layers kernels: host-side argument checks and
    size helpers, no launch."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)
    a = N.RoiGlueArgs()
    assert lib.dmh_roi_glue_fwd(ctypes.byref(a), one, None) != 0 and b"null pointer" in lib.dmh_last_error()
    a.y, a.dst_org = one, one
    a.B, a.C1, a.C2, a.sh, a.sw, a.hc, a.wc, a.H, a.W = 2, 8, 0, 10, 10, 6, 5, 16, 16      # odd window width
    assert lib.dmh_roi_glue_fwd(ctypes.byref(a), one, None) != 0 and b"even width" in lib.dmh_last_error()
    a.wc = 20                                                                            # window wider than its frame
    assert lib.dmh_roi_glue_bwd(ctypes.byref(a), one, one, None, None, 0, 0, None, 0, 0, None) != 0
    a.wc, a.y_org = 6, one                                                               # a region needs a whole-frame y
    assert lib.dmh_roi_glue_bwd(ctypes.byref(a), one, one, None, one, 4, 4, None, 0, 0, None) != 0
    assert b"whole-frame y" in lib.dmh_last_error()
    assert lib.dmh_roi_cost_partials_size(12, 174, 208) == 12 * 36
    assert lib.dmh_roi_cost_fwd(one, one, one, 2, 40, 40, 32, 64, one, one, one, None) != 0        # window taller than the frame
    assert lib.dmh_roi_crop(one, None, None, one, 2, 8, 16, 16, 6, 5, 0, one, None) != 0           # odd width
    assert lib.dmh_roi_crop(one, None, one, one, 2, 8, 16, 16, 6, 6, 0, one, None) != 0            # both src and g
    assert lib.dmh_roi_paste(one, one, 4, 4, one, 2, 8, 16, 16, 6, 6, one, None) != 0              # source smaller than the window
    assert lib.dmh_stem_bn_relu_pool_bwd_win(one, one, None, one, one, one, one, 2, 8, 16, 16, 6, 5, 4, 4, one, None) != 0
    assert lib.dmh_conv7x7s2_bwd_data_win(one, one, one, one, 2, 64, 3, 32, 64, 12, 15, 8, 10, one, None) != 0   # odd window
    assert lib.dmh_stem_conv_norm_fwd_win(one, one, one, 2, 32, 64, 20, 10, 0.45, 0.225, one, None) != 0        # taller than H/2
    assert lib.dmh_ssim_map(one, one, 6, 1, 8, one, None) != 0 and lib.dmh_edge_smooth_partials_size(2, 32, 96) == 2 * 2 * 3
    assert lib.dmh_edge_smooth(one, one, 2, 3, 1, 8, one, one, None) != 0


def test_strided_and_stem_weight_gradient_entry_points_without_gpu():
    """K20 / K21: workspace sizes (-1 for shapes the kernels do not take) and host-side argument checks, no launch."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)
    # layer2.0 at batch 32: 2 channel-block pairs x 256 pixel slices x 10 taps x 64 x 64
    assert lib.dmh_down_wrw_workspace_size(32, 64, 128, 80, 256) == 2 * 256 * 10 * 64 * 64
    assert lib.dmh_down_wrw_workspace_size(3, 64, 64, 6, 24) == 9 * 10 * 64 * 64            # nine row tiles: nine slices
    for bad in ((32, 48, 128, 80, 256), (32, 64, 96, 80, 256), (32, 64, 128, 81, 256), (32, 64, 128, 80, 100), (0, 64, 64, 8, 8)):
        assert lib.dmh_down_wrw_workspace_size(*bad) == -1, bad
    assert lib.dmh_down_wrw(one, None, None, 2, 64, 64, 8, 16, one, one, None, None) != 0 and b"null pointer" in lib.dmh_last_error()
    assert lib.dmh_down_wrw(one, one, one, 2, 64, 64, 8, 16, one, one, None, None) != 0            # gd without dwd
    assert lib.dmh_down_wrw(one, one, None, 2, 64, 64, 8, 12, one, one, None, None) != 0 and b"multiple of 8" in lib.dmh_last_error()
    # stem at batch 32, 320 x 1024: 20,480 row tiles -> 512 workgroups x 4 waves x 10 blocks of 32 x 32
    assert lib.dmh_stem_wrw_workspace_size(32, 320, 1024) == 512 * 4 * 10 * 1024
    assert lib.dmh_stem_wrw_workspace_size(3, 38, 72) == 30 * 4 * 10 * 1024
    assert lib.dmh_stem_wrw_workspace_size(2, 37, 72) == -1 and lib.dmh_stem_wrw_workspace_size(2, 38, 76) == -1
    assert lib.dmh_stem_wrw(one, one, 2, 38, 76, 0.45, 0.225, one, one, None) != 0 and b"multiple of 8" in lib.dmh_last_error()
    assert lib.dmh_stem_wrw(one, one, 2, 38, 72, 0.45, 0.0, one, one, None) != 0 and b"std" in lib.dmh_last_error()


def test_launch_forms_of_the_stem_and_head_convolutions_without_gpu():
    """K12 / K13 / K14 switch kernel form by grid size; the launchers and these host-only queries share ONE function per
    decision.  The forms at the workload's shapes: tests/test_gpu_stem_head_anchor.py asserts through the same
    queries which form each of its cases reached, so a threshold change cannot quietly uncover a form."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    # K12, image gradient: 16 x 64-pixel workgroups, KS = 4 below 2048 of them
    assert lib.dmh_conv7x7s2_bwd_data_ksplit(12, 320, 1024) == 1            # 12 x 20 x 16 = 3840
    assert lib.dmh_conv7x7s2_bwd_data_ksplit(2, 320, 1024) == 4             # 640
    assert lib.dmh_conv7x7s2_bwd_data_ksplit(12, 192, 640) == 4             # 12 x 12 x 10 = 1440
    assert lib.dmh_conv7x7s2_bwd_data_ksplit(40, 74, 660) == 1              # 40 x 5 x 11 = 2200
    assert lib.dmh_conv7x7s2_bwd_data_ksplit(12, 321, 1024) == -1
    # K13 backward-data: strips of 62 x 20 pixels of g_x, one wave per strip from 2048 strips on
    assert lib.dmh_conv3x3_head_bwd_data_nsplit(12, 16, 322, 1026) == 1     # 12 x 17 x 17 = 3468
    assert lib.dmh_conv3x3_head_bwd_data_nsplit(2, 16, 322, 1026) == 4      # 578
    assert lib.dmh_conv3x3_head_bwd_data_nsplit(128, 4, 44, 330) == 1       # 128 x 3 x 6 = 2304
    assert lib.dmh_conv3x3_head_bwd_data_nsplit(12, 18, 322, 1026) == -1
    # K13 weight gradient: strips of 62 x 40 outputs, channel groups doubled while strips x groups < 4096
    assert lib.dmh_conv3x3_head_wrw_strips(32, 16, 322, 1026, 0) == 32 * 8 * 17 == 4352
    assert lib.dmh_conv3x3_head_wrw_channel_groups(32, 16, 322, 1026, 0) == 1
    assert lib.dmh_conv3x3_head_wrw_strips(12, 16, 322, 1026, 0) == 1632
    assert lib.dmh_conv3x3_head_wrw_channel_groups(12, 16, 322, 1026, 0) == 4
    assert lib.dmh_conv3x3_head_wrw_channel_groups(2, 5, 87, 132, 0) == 1   # odd C: no split however few the strips
    assert lib.dmh_conv3x3_head_wrw_partials_size(32, 16, 322, 1026, 0) == 4352 * (16 * 9 + 1)
    assert lib.dmh_conv3x3_head_wrw_strips(0, 16, 322, 1026, 0) == -1
    # K13 forward: strips at pad 0 (C a multiple of 4), the LDS tile otherwise (C a multiple of 16)
    assert lib.dmh_conv3x3_head_fwd_form(12, 16, 322, 1026, 0) == 1
    assert lib.dmh_conv3x3_head_fwd_form(12, 20, 42, 64, 0) == 1
    assert lib.dmh_conv3x3_head_fwd_form(12, 16, 320, 1024, 1) == 0
    assert lib.dmh_conv3x3_head_fwd_form(12, 20, 42, 64, 1) == -1
    assert lib.dmh_conv3x3_head_fwd_form(1, 16, 8192, 4100, 0) == 0         # 2^29 elements: beyond the strips' byte offsets
    assert lib.dmh_conv3x3_head_fwd_form(1, 20, 8192, 4100, 0) == -1
    one = ctypes.c_void_p(16)       # rejected by the channel check, before any launch
    assert lib.dmh_conv3x3_head(one, one, None, 1, 20, 8192, 4100, 0, one, None) != 0 and b"multiple of 16" in lib.dmh_last_error()
    # K14: tiles of 4 x 32 outputs on at most 512 persistent workgroups
    assert lib.dmh_stem_conv_norm_fwd_tiles(12, 320, 1024) == 12 * 40 * 16
    assert lib.dmh_stem_conv_norm_fwd_workgroups(12, 320, 1024) == 512
    assert lib.dmh_stem_conv_norm_fwd_tiles(30, 46, 130) == 540 and lib.dmh_stem_conv_norm_fwd_workgroups(30, 46, 130) == 512
    assert lib.dmh_stem_conv_norm_fwd_tiles(3, 46, 130) == 54 and lib.dmh_stem_conv_norm_fwd_workgroups(3, 46, 130) == 54
    assert lib.dmh_stem_conv_norm_fwd_tiles(3, 45, 130) == -1
