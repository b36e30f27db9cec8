"""The import surface of nerf2mesh_amd/capture.py: every public name it defined before the lens models moved to lens.py and the COLMAP
codec to colmap_model.py is still found there, and a moved name is the very object of its new module.  Host code only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from nerf2mesh_amd import capture, colmap_model, lens   # noqa: E402

# dir() of the module before the split, without the underscore names and the modules it imports
STAYED = """Capture DepthSchedule FAR NEAR SparseDepth batch_from_uniforms_u8 batch_sparse_u8 batch_views box_downscale decode_lut decode_words
dense_depth_fill dense_depth_for depth_schedule_for fit_scale_bias intrinsics_row intrinsics_table nerf_matrix_to_ngp pack_rgba8 proj_matrix
rays_from_pixels resize_linear_at srgb_to_linear""".split()
TO_LENS = """LENS_BROWN LENS_FISHEYE LENS_MAX_ITER LENS_STEP ZOOM_MAX ZOOM_TOL border_taps_inside lens_distort lens_distort_f32 lens_row
lens_undistort undistort_bank undistort_depth undistort_source_f32 undistort_zoom""".split()
TO_COLMAP_MODEL = """COLMAP_DIRS COLMAP_MODELS center_poses decompose_projection quat_to_rotmat read_colmap_cameras read_colmap_images
read_colmap_points rotmat_to_quat""".split()
METHODS = "load_nerf load_colmap load_dtu from_arrays synthetic save_nerf save_colmap save_dtu view decode intrinsics_of check_device".split()


def test_every_public_name_is_still_there():
    names = STAYED + TO_LENS + TO_COLMAP_MODEL
    assert len(names) == len(set(names)) == 47
    assert [n for n in names if not hasattr(capture, n)] == []
    assert all(getattr(capture, n).__module__ == capture.__name__ for n in STAYED if callable(getattr(capture, n)))


def test_capture_keeps_its_methods():
    assert [m for m in METHODS if not callable(getattr(capture.Capture, m, None))] == []


def test_moved_names_are_the_objects_of_their_new_modules():
    assert [n for n in TO_LENS if getattr(capture, n) is not getattr(lens, n)] == []
    assert [n for n in TO_COLMAP_MODEL if getattr(capture, n) is not getattr(colmap_model, n)] == []
    assert capture.lens_distort is lens.lens_distort
