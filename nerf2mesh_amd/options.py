"""The reference's `opt` namespace: defaults of main.py:12-125 and its derived overrides (main.py:127-181)."""
from types import SimpleNamespace

_DEFAULTS = dict(
    O=False, workspace="workspace", seed=0, stage=0, ckpt="latest", fp16=False, sdf=False, tcnn=False, progressive_level=False,
    bound=2.0, scale=-1, offset=[0, 0, 0], mesh="", min_near=0.05,
    iters=30000, lr=1e-2, lr_vert=1e-4, pos_gradient_boost=1, cuda_ray=True, max_steps=1024, update_extra_interval=16,
    max_ray_batch=4096, grid_size=128, mark_untrained=False, dt_gamma=1 / 256, density_thresh=10, diffuse_step=1000,
    diffuse_only=False, background="random", enable_offset_nerf_grad=False,
    num_rays=4096, adaptive_num_rays=False, num_points=2 ** 18,
    lambda_density=0, lambda_entropy=0, lambda_tv=1e-8, lambda_depth=0.1, lambda_specular=1e-5, lambda_eikonal=0.1,
    lambda_rgb=1, lambda_mask=0.1,
    lambda_lpips=0, lambda_offsets=0.1, lambda_lap=0.001, lambda_normal=0, lambda_edgelen=0,
    contract=False, patch_size=1, trainable_density_grid=False, color_space="srgb", ind_dim=0, ind_num=500,
    ssaa=2, texture_size=4096, refine=False, gui=False,
    refine_steps_ratio=(0.1, 0.2, 0.3, 0.4, 0.5, 0.7), refine_size=0.01, refine_decimate_ratio=0.1, refine_remesh_size=0.02,   # main.py:111-114
    decimate_target=3e5,                                                                                                      # main.py:101
    clean_min_f=8, clean_min_d=5,                                                                                             # main.py:104-105
    cos_anneal_ratio=1.0, normal_anneal_epsilon=1e-4,
    fused_mlp=False,     # opt-in: fused MFMA field kernels (nerf2mesh_amd/fused.py) instead of nn.Linear calls
    enable_cam_near_far=False,     # main.py:40 (colmap mode): clamp every ray to its camera's sparse-point depth range
    enable_sparse_depth=False,     # main.py:41 (colmap mode): one step in ten supervises the depth of one view's sparse keypoints (lambda_depth)
    enable_dense_depth=False,      # main.py:44 (colmap mode): every ray of every step carries a depth target from the view's calibrated depth map (lambda_depth)
    data_format="nerf",            # main.py:36: "nerf" | "colmap" | "dtu" (tools/train_capture.py; capture.Capture.load_nerf / load_colmap / load_dtu)
    per_view_intrinsics=False,     # not a reference option (it always keeps intrinsics [N,4]): a COLMAP set whose images use different cameras is
                                   # loaded with one (fx, fy, cx, cy) row per view (capture.Capture.per_view_intrinsics); "dtu" implies it
    undistort=False,               # not a reference option (it ignores lens distortion): a COLMAP set is resampled once, at load, to a pinhole camera with
                                   # its cameras' lens coefficients (capture.Capture.load_colmap(undistort=True), n2m_capture_undistort)
    lambda_ssim=0,       # not a reference option (its structural term is LPIPS on patches, --lambda_lpips, which needs VGG weights): weight of
                         # 1 - SSIM of the whole frame in stage 1 (metrics.ssim); > 0 selects the torch-graph head of trainer.Stage1Trainer
    lambda_patch_ssim=0,  # not a reference option: weight of 1 - SSIM over the P x P patches of a stage-0 batch (metrics.ssim_patches); needs
                         # patch_size >= 11 and selects the unfused loss branch of trainer.Stage0Trainer.  A name of its own: lambda_ssim is handed
                         # to both stages' options by tools/evaluate.py and stage 0 ignores it
    lambda_distort=0,    # not a reference option (nerf2mesh dropped the term its ancestor torch-ngp carried): weight of the distortion loss of the
                         # ray weights in stage 0 (losses.distortion_loss); > 0 selects trainer.Stage0Trainer, the step executor
                         # does not carry the term
    distort_space="linear",   # not a reference option: the coordinate the sample intervals are normalised in, "linear" (t) | "disparity" (1 / t,
                         # mip-NeRF 360's choice on unbounded scenes)
    optimize_poses=False,     # not a reference option: stage 0 trains a correction (omega, tau) per camera next to the field
                         # (pose_refine.PoseRefiner); needs a captured set and the unfused field, selects trainer.Stage0Trainer
    lr_pose=1e-3,        # not a reference option: the learning rate of those corrections (Adam of its own, the field's schedule)
    mesh_method="density",    # not a reference option (it always thresholds the density lattice): how export_stage0 finds the inner mesh, "density" |
                         # "tsdf" (TSDF fusion of the depth rendered at every training camera: tsdf.py; needs a captured set)
    tsdf_trunc=0,        # not a reference option: the truncation distance of that fusion in world units; 0: four lattice spacings
    tsdf_carve=False,    # not a reference option: rays that stop at nothing (opacity < 0.05) mark every point along them as empty
    tsdf_alpha_min=0.5,  # not a reference option: the least opacity at which a ray's depth counts as a surface observation
    camera_traj="",    # main.py:28: the test-time camera path, "" (interpolate between random training views) | "circle" (camera_path.path_for)
    scene="lego",        # not a reference option: which synthetic stand-in the drivers render (nerf2mesh_amd/synthetic.py: "lego" | "garden")
)


def make_options(**overrides):
    """opt = make_options(O=True, bound=1, dt_gamma=0) reproduces `main.py -O --bound 1 --dt_gamma 0`."""
    unknown = set(overrides) - set(_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s): {sorted(unknown)}")
    o = SimpleNamespace(**{**_DEFAULTS, **overrides})
    o.cuda_ray = True                                   # main.py:127
    if o.O:                                             # main.py:129-136
        o.fp16 = True
        o.mark_untrained = True
        o.adaptive_num_rays = True
        o.refine = True
    if o.sdf:                                           # main.py:138-153
        o.density_thresh = 0.001
        if o.stage == 0:
            o.progressive_level = True
        if o.bound > 1:
            o.contract = True
        o.enable_offset_nerf_grad = True
        o.refine_decimate_ratio = 0                     # main.py:151-153: the SDF recipe only re-meshes
        o.refine_size = 0
    if o.contract:                                      # main.py:155-157
        o.mark_untrained = False
    o.refine_steps = [int(round(x * o.iters)) for x in o.refine_steps_ratio]   # main.py:181
    return o
