"""Single-file inference, the reference's ``test.py`` (:94-164) + ``utils.eval_notruth`` (utils.py:391-424): a camera frame
(``.pcd``) or a dataset record (``.p``) in, the ``*_data_predict/*.p`` file of collision-filtered grasps out.

``GraspDetector.detect`` chains ``ingest`` (transform, crop, colour gains and the ``np.random.choice`` rows on the device)
-> ScoreNet -> ``get_grasp_allobj`` -> the region network -> ``eval_collision.eval_test`` on each of the four grasp sets,
inside one ``np_random.deferred()`` block.  What it adds to the host reads the grouping and region stages already make is a
4-byte read of the kept count before the collision filter and the final download.  Run as a module for ``test.py``'s
``main()``:

    python -m regnet_for_3d_grasping_amd.detect --folder DIR [--file NAME] --load-score-path S --load-region-path R

With ``select`` (``--top-k`` / ``--nms-translation`` / ``--nms-rotation`` / ``--select-from``) the record additionally carries the
best distinct grasps of one of the four sets: pose non-maximum suppression + top-K on the device (``grasp_select.pose_nms``),
before the final download.  Without it nothing changes.

With ``transform="auto"`` (``--auto-table``, ``--table-range LO HI``, ``--plane-threshold``) the camera -> table transform is not
the reference lab's hard-coded camera pose but is estimated on every camera frame: the dominant plane found on the device
(``table_plane.estimate_plane``) becomes the table at ``eval_params[2]``, and the record additionally carries ``TABLE_KEYS``.
``GraspDetector.calibrate(frame)`` does it once and keeps the transform.  Dataset records are never transformed.

A camera frame may also be a ``depth_frame.DepthFrame`` (a ``.npz`` file: depth image, optional colour image, intrinsics): it
becomes the ``(xyz, rgb)`` pair on the device (``depth_frame.to_cloud``; ``depth`` / ``--depth-range``, ``--edge-threshold``,
``--min-neighbours``, ``--occlusion-margin``, ``--keep-uncoloured`` set its filter) and takes the camera-frame path from there.

With ``segment`` (``--segment``, ``--cluster-tolerance``, ``--min-object-points``, ``--max-objects``, ``--top-k-per-object``) the
points above the table are clustered into objects on the device (``segment.cluster_points``), every grasp of one set is given
the object it belongs to, and the selection may be per object; the record additionally carries ``SEGMENT_KEYS``.

A camera frame may also be a ``fusion.MultiView`` (a ``.npz`` file with a ``views`` entry: the depth frames of up to 8 cameras
and their poses): the views are merged into one evenly sampled cloud on the device (``fusion.voxel_merge``; ``fuse`` / ``--voxel``,
``--max-voxels``, ``--min-voxel-points`` set the voxel grid) and take the camera-frame path from there, ``transform="auto"``
included; the record additionally carries ``FUSE_KEYS``.  With ``register`` (``--refine-poses``, ``--icp-distance``,
``--icp-iterations``, ``--icp-stride``, ``--icp-association``, ``--icp-window``, ``--icp-normal-angle``) the views' poses are
first corrected against the first view on the device (``fusion.refine_poses``: point-to-plane ICP, by the nearest point or by a
lookup in the first view's depth image, one more host read for all views) and the record additionally carries
``REGISTER_KEYS``.  Without it nothing changes.

With ``approach`` (``--approach``, ``--approach-standoff``, ``--approach-from``, ``--friction-angle``, ``--min-clearance``,
``--min-contact``) every grasp of one collision-filtered set is analysed on the device (``approach.analyse``): how far the hand can
retreat straight back before it touches the cloud, the extent and offset of the object between the fingers, the opening to
command, the contact check and the pre-grasp point; the record additionally carries ``APPROACH_KEYS``, row-aligned with that set,
and with ``min_clearance`` / ``min_contact`` the selection sees only the rows that pass.  Without it nothing changes.
With ``space="volume"`` (``--approach-space``, ``--approach-unseen``, ``--approach-step``, ``--approach-margin``) the hand is held against the TSDF volume instead (``approach.analyse_volume``): ``APPROACH_VOLUME_KEYS`` follow.
With ``field=True`` (``--approach-field``, ``--min-margin``) the volume's distance field is built once per frame
(``tsdf.Volume.distance_field``) and ``APPROACH_FIELD_KEYS`` follow those: how much room the hand has.  With
``field_signed=True`` (``--approach-signed``) the field is signed -- a margin below zero is minus a penetration depth -- and
``grasp_colliding`` (B,2) int32, the hand's and the swept hand's samples inside an obstacle, follows; ``field_max_distance``
(``--approach-field-cap``) caps the field's distances, which bounds its cost.
With ``retreat`` (``--approach-retreat``, ``--retreat-length``, ``--retreat-steps``, ``--retreat-tilt``, ``--retreat-up``,
``--min-retreat``) the hand at its final pose is moved along a fan of retreat directions against that field
(``approach.retreat_fan``) and ``APPROACH_RETREAT_KEYS`` follow: the picked direction, its free length, margin and pre-grasp point.
With ``paths`` (``--approach-paths``, ``--path-turn``, ``--path-length``, ``--path-steps``, ``--path-pivot``, ``--min-path``) the hand
is taken through candidate trajectories of POSES against that field (``approach.check_paths``: the fan's five directions and four
turns of the straight retreat) and ``APPROACH_PATH_KEYS`` follow; ``min_path`` selects on the picked path's certified length.  The
fan and the paths are independent.
With ``push`` (``--approach-push``, ``--push-target``, ``--push-max-shift``, ``--push-iterations``, ``--push-axes``,
``--push-keep``) every hand that has less than the target margin is first moved along the signed field's gradient
(``approach.push_out``); a grasp that move freed is analysed at its moved centre and ``APPROACH_PUSH_KEYS`` follow.

With ``denoise`` (``--denoise``, ``--outlier-mode``, ``--outlier-radius``, ``--outlier-min-neighbours``, ``--outlier-knn``,
``--outlier-max-radius``, ``--outlier-std-ratio``) the cloud of a camera frame -- an ``(xyz, rgb)`` pair, a depth frame's or a
multi-view merge's -- loses its outliers on the device (``outliers.filter_cloud``: the reference's radius filter, the statistical
filter, or both) before the table plane is estimated and the frame is cropped; the record additionally carries ``DENOISE_KEYS``.
Dataset records never see it.  Without it nothing changes and the module is not imported.

With ``volume`` (``--tsdf``, ``--tsdf-voxel``, ``--tsdf-trunc``, ``--tsdf-origin``, ``--tsdf-dims``, ``--tsdf-min-weight``) a
``fusion.MultiView`` is not merged point by point but integrated view by view into a truncated signed distance volume on the
device, whose surface becomes the cloud (``tsdf.fuse_volume``): noise along the viewing rays averages out and what one view sees
another may declare empty; ``register`` applies as before.  The record then carries ``TSDF_KEYS`` (and ``REGISTER_KEYS``) instead of
``FUSE_KEYS``.  Without it nothing changes and the module is not imported.

With ``track`` (``--track``, ``--track-near``, ``--track-far``, ``--track-step``, ``--track-max-translation``,
``--track-max-rotation``; coarse to fine with ``--track-levels``, ``--track-level-iterations``, ``--track-dist-scale`` and
``--track-smooth RADIUS SIGMA_SPACE SIGMA_DEPTH``, and the record of a frame registered that way also carries ``track_levels``) the ``DepthFrame``s handed to ``detect`` -- on the command line the folder's ``.npz`` frames in the order
of their names -- are one moving camera whose pose is not given: each is registered against the model view raycast from the
volume at the last pose and integrated at the pose found (``tsdf.Tracker``), and the volume's surface is the frame's cloud.  The
record then carries ``TSDF_KEYS`` and ``TRACK_KEYS``.  Without it nothing changes and the module is not imported.

With ``mesh`` (``--tsdf-mesh``; beside ``volume`` or ``track``) the volume's surface is taken as a triangle mesh
(``tsdf.Volume.extract_mesh``) and the record also carries ``TSDF_MESH_KEYS``; ``--tsdf-mesh-ply`` writes it as ``NAME.ply`` beside
the record.  Without it no launch, no allocation and no key changes.  With ``mesh_cell`` (``--tsdf-mesh-cell M``) that mesh is
simplified on the device first (``tsdf.Mesh.simplify``, vertex clustering on cells of M metres): ``TSDF_MESH_KEYS`` and the
``.ply`` then hold the simplified mesh and ``tsdf_mesh_report`` is added; the networks still see the full surface.
"""
import argparse
import contextlib
import glob
import io
import os
import pickle

import numpy as np

# test.py:61-81, :90
ALL_POINTS_NUM = 25600
OBJ_CLASS_NUM = 43
WIDTH, HEIGHT, DEPTH = 0.08, 0.010, 0.06
TABLE_HEIGHT = 0.75
CENTER_NUM = 4000
MODEL_PARAMS = [OBJ_CLASS_NUM, 256, 64, 0.5, DEPTH, 10]
TEST_PARAMS = [CENTER_NUM, 0.5, 256, 0.1, 2048, 0.8, WIDTH, HEIGHT, DEPTH]
GRIPPER_PARAMS = [WIDTH, HEIGHT, DEPTH]
EVAL_PARAMS = [DEPTH, WIDTH, TABLE_HEIGHT, 0, CENTER_NUM]
USE_THETA = True
RESULT_KEYS = ("points", "colors", "scores", "grasp_stage2", "grasp_stage3_stage2", "grasp_stage3", "grasp_stage3_score")
SELECT_KEYS = ("grasp_selected", "grasp_selected_index")       # added to the record when the detector has ``select``
TABLE_KEYS = ("table_transform", "table_plane")                # added when the transform is estimated per frame ("auto")
SEGMENT_KEYS = ("point_object", "object_size", "object_bbox", "grasp_object")    # added when the detector has ``segment``
SEGMENT_SELECT_KEYS = SELECT_KEYS + ("grasp_selected_object",)                  # ... with ``top_k_per_object``
FUSE_KEYS = ("fuse_num", "fuse_views")                          # added when the frame was a ``fusion.MultiView``
REGISTER_KEYS = ("fuse_poses", "fuse_register")                 # ... and the detector has ``register``
APPROACH_KEYS = ("grasp_clearance", "grasp_width", "grasp_offset", "grasp_opening", "grasp_contact",
                 "grasp_pregrasp")                             # added when the detector has ``approach``: one row per source grasp
APPROACH_VOLUME_KEYS = ("grasp_clearance_seen", "grasp_clearance_safe", "grasp_unseen",
                        "grasp_solid_hand")                    # ... right after them when its ``space`` is "volume"
APPROACH_FIELD_KEYS = ("grasp_margin_hand", "grasp_margin_sweep")   # ... and right after those when it has ``field``
APPROACH_SIGNED_KEYS = ("grasp_colliding",)   # ... and after those when the field is signed: (B,2) int32, hand and sweep
APPROACH_RETREAT_KEYS = ("grasp_retreat_index", "grasp_retreat_length", "grasp_retreat_margin", "grasp_retreat_direction",
                         "grasp_retreat_pregrasp", "grasp_retreat_steps")   # ... and after the field keys with ``retreat``: the
                                                  # picked direction's row, free length, margin, vector and pre-grasp point (in the
                                                  # grasps' frame), and the (B,R) free steps of all directions
APPROACH_PATH_KEYS = ("grasp_path_index", "grasp_path_steps", "grasp_path_certified", "grasp_path_margin",
                      "grasp_path_pose")          # ... and after those with ``paths``: the picked path's row, the (B,R) free and
                                                  # certified steps of all paths, the picked path's margin and the pre-grasp POSE
                                                  # (B,12): rows 0..2 of the hand's pose at the picked path's last free step, in
                                                  # the grasps' frame
APPROACH_PUSH_KEYS = ("grasp_push_status", "grasp_push_shift", "grasp_push_margin",
                      "grasp_push_centre")        # ... and after those with ``push``: the push-out's status (an index into
                                                  # ``hand_adjust.STATUS``), the (B,3) move in the hand's LOCAL frame, the margin
                                                  # at its last iterate, and the (B,3) centre the grasp was analysed at, in the
                                                  # grasps' frame: the moved one where the status is FREED
TSDF_KEYS = ("tsdf_num", "tsdf_counts")                        # added when the frame was a ``MultiView`` and the detector has ``volume``
TRACK_KEYS = ("track_pose", "track_status", "track_report")    # added beside ``TSDF_KEYS`` when the detector has ``track``
TSDF_MESH_KEYS = ("tsdf_triangles", "tsdf_vertices", "tsdf_vertex_normals",
                  "tsdf_vertex_colors")                        # added after them when the detector has ``mesh``
TSDF_MESH_REPORT_KEYS = ("tsdf_mesh_report",)                  # added after them when the detector has ``mesh_cell``
VIEW_KEYS = ("view_pose", "view_gain", "view_rays", "view_order",
             "view_order_gain")                                 # added last when the detector has ``view``: the next-best view
DENOISE_KEYS = ("denoise_num",)                                 # added when the detector has ``denoise`` and the frame was a camera frame


def save_path_for(pc_path, real_data):
    """test.py:143-145: ``_data`` -> ``_data_predict`` anywhere in the path; camera frames also ``.pcd`` -> ``.p``, and a depth
    frame's trailing ``.npz`` -> ``.p``."""
    path = pc_path.replace("_data", "_data_predict")
    if real_data and path.endswith(".npz"):
        return path[:-len(".npz")] + ".p"
    return path.replace(".pcd", ".p") if real_data else path


class GraspDetector:
    """``GraspDetector(score_net, region_net)``: both networks on one GPU, in eval mode for the call.  ``params`` /
    ``gripper_params`` / ``eval_params`` are test.py's lists (:78-81, :90; ``eval_params[3]`` is the GPU index of the
    collision filter and follows the networks' device).  ``transform`` / ``bounds``: see ``ingest.ingest_frame``.
    ``select``: None, or a ``grasp_select.SelectParams`` / a dict of its fields (``source``, ``top_k``,
    ``translation_thresh``, ``rotation_thresh_deg``, ``symmetric``): the record then also carries ``grasp_selected`` (k,8),
    the best distinct grasps of the collision-filtered set ``source``, and ``grasp_selected_index`` (k,) int64, their rows in
    that set.  ``transform``: a 4x4 (default ``ingest.table_frame_transform()``), or ``"auto"`` / a dict of
    ``table_plane.estimate_plane`` keywords: the table plane is then estimated on every camera frame and placed at
    ``eval_params[2]``, and the record also carries ``table_transform`` (4,4) float64 and ``table_plane`` (5,) float64 =
    normal, offset, rms.  ``depth``: None, or a ``depth_frame.DepthParams`` / a dict of its fields: how a ``DepthFrame`` handed
    to ``ingest`` / ``detect`` becomes a cloud (range, edge filter, occlusion test); other frames never see it.
    ``segment``: None, or a ``segment.SegmentParams`` / a dict of its fields: the record's points above the table are clustered
    into objects and the record also carries ``point_object`` (count,) int32, ``object_size`` (K,) int32, ``object_bbox`` (K,6)
    float32 and ``grasp_object`` (k_source,) int32, the object of every grasp of the source set (-1: none); with
    ``top_k_per_object`` the selection is the best distinct grasps of every object and ``grasp_selected_object`` (k,) int32
    names each one's object; it replaces the per-frame selection: ``select``'s source and thresholds apply, its ``top_k`` does
    not.  ``fuse``: None, or a ``fusion.FuseParams`` / a dict of its fields (``voxel``, ``origin``, ``max_voxels``, ``min_count``):
    how a ``fusion.MultiView`` handed to ``ingest`` / ``detect`` is merged into one cloud; the record then also carries
    ``fuse_num`` (4,) int32 = (merged points, rows merged, rows dropped, overflow) and ``fuse_views`` (views,) int64, the merged
    points each view contributed to.  Other frames never see it.  ``register``: None, or a ``registration.IcpParams`` / a dict of
    its fields (``max_dist``, ``iterations``, ``stride``, ``min_pairs``, ...): the poses of a ``MultiView`` are refined against its
    first view before the merge (``fusion.refine_poses``) and the record also carries ``fuse_poses`` (views,4,4) float64, the
    poses the merge used, and ``fuse_register`` (views,5) float64 = (status, iterations, pairs, rms first, rms last) per view.
    ``approach``: None, or an ``approach.ApproachParams`` / a dict of its fields (``source``, ``standoff``, ``friction_deg``,
    ``min_clearance``, ``min_contact``, ...): every grasp of the collision-filtered set ``source`` is analysed against the cloud
    and the record also carries, one row per grasp of that set, float32 ``grasp_clearance`` (k,) [m], ``grasp_width`` (k,),
    ``grasp_offset`` (k,), ``grasp_opening`` (k,), ``grasp_contact`` (k,) and ``grasp_pregrasp`` (k,3).  With ``min_clearance`` /
    ``min_contact`` the per-frame or per-object selection sees only the rows that pass (its source must then be the analysed
    set); ``grasp_selected_index`` still holds rows of the full set, and the four sets are never shortened.  With its
    ``space="volume"`` (the detector then needs ``volume`` or ``track``, and the frame must be one that fills the volume, else a
    ValueError) the grasps are held against the TSDF volume and its surface's normals (``approach.analyse_volume``):
    ``grasp_clearance`` is the clearance of the ``unseen`` policy, and right after the six come float32 ``grasp_clearance_seen``,
    ``grasp_clearance_safe``, ``grasp_unseen`` (k,) and int32 ``grasp_solid_hand`` (k,).
    ``denoise``: None, or an ``outliers.OutlierParams`` / a dict of its fields (``mode``, ``radius``, ``min_neighbours``, ``knn``,
    ``max_radius``, ``std_ratio``): the cloud of a camera frame is filtered on the device after ``to_cloud`` / ``fuse_frames`` and
    before the table plane and the crop -- the removed rows become NaN rows, which both treat as absent -- and the record also
    carries ``denoise_num`` (5,) int32, the rows that were no point, had too few rows within ``radius``, fewer than ``knn`` rows
    within ``max_radius``, a mean distance above the threshold, and were kept.  Records and ``ingest.Frame``s never see it.
    ``volume``: None, or a ``tsdf.TsdfParams`` / a dict of its fields (``voxel``, ``trunc``, ``origin``, ``dims``, ``max_weight``,
    ``min_weight``, ``max_points``): a ``MultiView`` goes through ``tsdf.fuse_volume`` instead of ``fusion.fuse_frames`` -- the views
    are integrated in their order into a TSDF volume, kept between frames, and its surface is the cloud -- and the record carries
    ``tsdf_num`` (4,) int32 = (surface rows, kept candidates, observed voxels, overflow) and ``tsdf_counts`` (views,4) int32, per
    view the voxels updated, not in view, without depth and behind the surface, and with ``register`` ``fuse_poses`` /
    ``fuse_register`` as above, in place of ``fuse_num`` / ``fuse_views``.  Together with ``fuse`` it is a ValueError.
    ``track``: None, or a ``tsdf.TrackParams`` / a dict of its fields (``near``, ``far``, ``step``, ``max_translation``,
    ``max_rotation``, ``min_hit_share``, ``max_dist``, ``iterations``, ...): the ``DepthFrame``s handed to ``detect`` are the
    frames of ONE moving camera whose pose is not given.  Each goes through the detector's ``tsdf.Tracker`` (``tracker``; its
    volume is ``volume``'s, ``tsdf.TsdfParams()`` when that is absent, and is never reset between frames): registered against
    the model view from the last pose and integrated at the pose found, and the surface of the volume as it then stands is the
    cloud, in the frame of the FIRST camera.  The record carries ``tsdf_num`` as above, ``tsdf_counts`` (1,4) int32 (zeros for
    a frame that was LOST), ``track_pose`` (4,4) float64 camera-to-common, ``track_status`` () int32 (0 FIRST, 1 TRACKED, 2
    LOST) and ``track_report`` (5,) float64 = (status, iterations, pairs, rms first, rms last) of the registration (NaN for
    the first frame).  Together with ``fuse``, or for a ``MultiView`` (its views carry poses), it is a ValueError.
    ``mesh``: True (or a ``"mesh": True`` entry in the ``volume`` / ``track`` dict), with ``volume`` or ``track``: the surface is
    taken by ``tsdf.Volume.extract_mesh`` and the record also carries ``tsdf_triangles`` (Kt,3) int32 -- rows of
    ``tsdf_vertices`` per triangle, in cell order, normals out of the solid -- and float32 ``tsdf_vertices``,
    ``tsdf_vertex_normals``, ``tsdf_vertex_colors`` (K,3): the WHOLE surface of the volume in the common frame, before the crop
    chooses rows.  ``mesh_ply``: ``detect_file`` also writes them as a binary PLY beside the record.  Without ``mesh`` nothing
    is launched or allocated for it.
    ``mesh_cell`` [m] (implies ``mesh``; may ride in the dicts too): the mesh goes through ``tsdf.Mesh.simplify(cell=mesh_cell)``
    on the device before it is downloaded -- the four mesh keys and the PLY are then the simplified mesh, whose triangles ascend
    by the full mesh's rows, and ``tsdf_mesh_report`` (12,) int32 is ``SimplifiedMesh.report``.  The cloud the networks see is
    the full surface either way.  Without it every key and file is what it is without the option.
    ``view``: None, or a ``view_plan.ViewParams`` / a dict of its fields (``width``, ``height``, ``near``, ``far``, ``step``,
    ``max_unknown``, ``top_k``, ``min_gain``, ``interest``, ``azimuths``, ``elevations``, ``radius``, ...), with ``volume`` or
    ``track`` (anything else is a ValueError): where the camera should go next.  Candidate poses orbit the centroid of the kept
    grasps of the analysed (else the selected) set -- the volume's centre when there are none -- and are ranked by the unobserved
    voxels of the frame's volume each would reveal (``view_plan.view_gain``); ``interest="grasps"`` (it needs ``approach`` with
    ``space="volume"``) counts only those inside the swept hands of the analysed grasps.  The record also carries, last,
    ``view_pose`` (P,4,4) float64 camera-to-common in the volume's frame, ``view_gain`` (P,) int32, ``view_rays`` (P,4) int32,
    ``view_order`` (K,) int32, the joint greedy pick (-1: nothing more to gain), and ``view_order_gain`` (K,) int32.  Without it
    nothing is launched, allocated or imported for it and every record is what it was."""

    def __init__(self, score_net, region_net, params=TEST_PARAMS, gripper_params=GRIPPER_PARAMS, eval_params=EVAL_PARAMS,
                 transform=None, bounds=None, num_points=ALL_POINTS_NUM, use_theta=USE_THETA, select=None, depth=None, segment=None,
                 fuse=None, register=None, approach=None, denoise=None, volume=None, track=None, mesh=False, mesh_ply=False,
                 mesh_cell=None, view=None):
        from . import depth_frame, fusion, grasp_select, ingest, registration
        from . import segment as segment_mod
        self.fuse = fusion.FuseParams.coerce(fuse)
        self.register = registration.IcpParams.coerce(register)
        self.fused = None                         # the fusion.Fused of the last frame, when it was a MultiView
        self.segment = segment_mod.SegmentParams.coerce(segment)
        self.select = grasp_select.SelectParams.coerce(select)
        self.depth = depth_frame.DepthParams.coerce(depth)
        self.approach = self.approach_source = None
        if approach is not None:                  # (the module is not even imported without it)
            from . import approach as approach_mod
            self.approach = approach_mod.ApproachParams.coerce(approach)
            selected = self.select.source if self.select is not None else "grasp_stage3"
            self.approach_source = self.approach.source or selected
            if self.segment is not None and self.segment.top_k_per_object is not None:
                selected = self.segment.source or selected
            if self.approach.filters() and self.approach_source != selected:
                raise ValueError("approach: min_clearance / min_contact filter the selection, whose source is %s, not %s"
                                 % (selected, self.approach_source))
        self.mesh = bool(mesh) or bool(mesh_ply)  # the surface as a triangle mesh; may also ride in the volume / track dict
        self.mesh_ply = bool(mesh_ply)
        self.mesh_cell = mesh_cell                # the cell edge [m] the mesh is simplified with, None: the full mesh
        if isinstance(volume, dict) and ("mesh" in volume or "mesh_cell" in volume):
            volume = dict(volume)
            self.mesh = bool(volume.pop("mesh", False)) or self.mesh
            self.mesh_cell = volume.pop("mesh_cell", self.mesh_cell)
        if isinstance(track, dict) and ("mesh" in track or "mesh_cell" in track):
            track = dict(track)
            self.mesh = bool(track.pop("mesh", False)) or self.mesh
            self.mesh_cell = track.pop("mesh_cell", self.mesh_cell)
        if self.mesh_cell is not None:
            self.mesh_cell = float(self.mesh_cell)
            if not (self.mesh_cell > 0.0 and np.isfinite(self.mesh_cell)):
                raise ValueError("mesh_cell: the cell edge must be positive and finite")
            self.mesh = True
        if self.mesh and volume is None and track is None:
            raise ValueError("mesh: the triangle mesh is that of the detector's TSDF volume; give volume=... or track=...")
        self.volume = self.tsdf_volume = None     # the parameters, and the tsdf.Volume kept between frames
        self.distance_field = None                # the tsdf.DistanceField of approach.field, its buffers kept between frames
        if volume is not None:                    # (the module is not even imported without it)
            if fuse is not None:
                raise ValueError("volume: a MultiView is either merged (fuse) or integrated into a volume, not both")
            from . import tsdf
            self.volume = tsdf.TsdfParams.coerce(volume)
        self.track = self.tracker = None          # the parameters, and the tsdf.Tracker kept between frames
        if track is not None:                     # (the module is not even imported without it)
            if fuse is not None:
                raise ValueError("track: the frames of a moving camera are integrated into a volume, not merged (fuse)")
            from . import tsdf
            self.track = tsdf.TrackParams.coerce(track)
            if self.volume is None:
                self.volume = tsdf.TsdfParams()
        if self.approach is not None and self.approach.space == "volume" and self.volume is None:
            raise ValueError("approach: space=\"volume\" analyses the detector's TSDF volume; give volume=... or track=...")
        self.view = self.view_camera = self.approach_result = None
        if view is not None:                      # (the module is not even imported without it)
            if self.volume is None:
                raise ValueError("view: the next-best view is planned in the detector's TSDF volume; give volume=... or track=...")
            from . import view_plan
            self.view = view_plan.ViewParams.coerce(view)
            if self.view.interest == "grasps" and (self.approach is None or self.approach.space != "volume"):
                raise ValueError("view: interest=\"grasps\" counts the unseen space of the analysed hands; give "
                                 "approach=ApproachParams(space=\"volume\")")
        self.denoise = None
        if denoise is not None:                   # (the module is not even imported without it)
            from . import outliers
            self.denoise = outliers.OutlierParams.coerce(denoise)
        self.score_net, self.region_net = score_net, region_net
        self.params, self.gripper_params, self.eval_params = list(params), list(gripper_params), list(eval_params)
        self.auto_table = None                    # estimate_plane's keywords when the transform is estimated per frame
        if isinstance(transform, str):
            if transform != "auto":
                raise ValueError("transform must be a 4x4, None, \"auto\" or a dict of estimate_plane keywords")
            transform = {}
        if isinstance(transform, dict):
            self.auto_table, transform = dict(transform), None
        self.transform = ingest.table_frame_transform() if transform is None else np.asarray(transform, dtype=np.float64)
        self.table = None                         # (transform, plane) of the last automatically calibrated frame
        self.bounds = ingest.DEFAULT_BOUNDS if bounds is None else tuple(bounds)
        self.num_points, self.use_theta = int(num_points), use_theta
        self.device = next(score_net.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("GraspDetector: the networks must be on a GPU (no CPU path)")

    def ingest(self, frame):
        """``frame``: an ``ingest.Frame``, an ``(xyz, rgb)`` pair of a camera frame, a ``depth_frame.DepthFrame``, a
        ``fusion.MultiView`` or a record dict -> ``ingest.Frame``; what was found on the way rides on it: ``fused`` (the
        ``fusion.Fused`` of a ``MultiView``, or with ``volume`` its ``tsdf.Surface``), ``table`` (the (transform, plane)
        estimated in the frame) and ``denoised`` (the
        ``outliers.Filtered`` of a camera frame's cloud when the detector has ``denoise``), else None."""
        from . import depth_frame, fusion, ingest
        from ._frame_util import to_device
        if isinstance(frame, ingest.Frame):
            return frame
        if isinstance(frame, dict):
            return ingest.ingest_record(frame, self.num_points, self.device)
        fused = table = denoised = tracked = meshed = None
        if self.view is not None:                 # the camera whose field of view the candidates get: the (first) depth frame's
            first = frame.frames[0] if isinstance(frame, fusion.MultiView) else frame
            self.view_camera = None
            if isinstance(first, depth_frame.DepthFrame):
                self.view_camera = (first.intrinsics, int(first.depth.shape[1]), int(first.depth.shape[0]))
        if self.track is not None and isinstance(frame, fusion.MultiView):
            raise ValueError("track: a MultiView's views carry their poses; track takes the DepthFrames of one moving camera")
        if self.track is not None and isinstance(frame, depth_frame.DepthFrame):   # one blocking read: the registration's state
            from . import tsdf
            if self.tracker is None:
                self.tracker = tsdf.Tracker(self.volume, self.track, self.device, depth_params=self.depth)
                self.tsdf_volume = self.tracker.volume
            tracked = self.tracker.track(frame)
            if self.mesh:
                meshed = self.tracker.volume.extract_mesh()
                fused = meshed.surface
                if self.mesh_cell is not None:
                    meshed = meshed.simplify(cell=self.mesh_cell)
            else:
                fused = self.tracker.volume.extract()
            frame = fused.cloud()
        elif isinstance(frame, fusion.MultiView) and self.volume is not None:     # integrated on the device, no host read
            from . import tsdf
            fused = tsdf.fuse_volume(frame, self.depth, self.volume, device=self.device, register=self.register,
                                     volume=self.tsdf_volume, mesh=self.mesh, mesh_cell=self.mesh_cell)
            if self.mesh:
                fused, meshed = fused
            self.tsdf_volume = fused.volume
            frame = fused.cloud()
        elif isinstance(frame, fusion.MultiView):          # merged on the device, no host read; the rows beyond the merged
            fused = fusion.fuse_frames(frame, self.depth, self.fuse, device=self.device,         # points are NaN rows
                                       register=self.register)
            frame = fused.cloud()
        elif isinstance(frame, depth_frame.DepthFrame):    # on the device, no host read; draws nothing from numpy's stream
            frame = depth_frame.to_cloud(frame, self.depth, device=self.device)
        xyz, rgb = frame
        if self.denoise is not None:              # on the device, no host read; draws nothing from numpy's stream
            from . import outliers
            xyz, rgb = to_device(xyz, self.device), to_device(rgb, self.device)
            denoised = outliers.filter_cloud(xyz, self.denoise)
            xyz, rgb = denoised.apply(xyz, rgb)
        transform = self.transform
        if self.auto_table is not None:           # draws nothing from numpy's stream; one 96-byte read
            from . import table_plane
            xyz, rgb = to_device(xyz, self.device), to_device(rgb, self.device)
            table = table_plane.calibrate(xyz, self.eval_params[2], **self.auto_table)
            transform = table[0]
        fr = ingest.ingest_frame(xyz, rgb, transform, self.bounds, self.num_points, self.device)
        fr.fused, fr.table, fr.denoised, fr.tracked, fr.meshed = fused, table, denoised, tracked, meshed
        return fr

    def calibrate(self, frame, **estimate_kwargs):
        """Estimate the table plane of ``frame`` (an ``(xyz, rgb)`` pair or just ``xyz``) once and keep the transform for every
        later call: ``self.transform`` is replaced and the per-frame estimation, if it was on, is switched off.
        ``estimate_kwargs`` default to the ones the detector was built with.  -> (transform, plane)."""
        from . import table_plane
        xyz = frame[0] if isinstance(frame, (tuple, list)) else frame
        kwargs = dict(self.auto_table or {})
        kwargs.update(estimate_kwargs)
        kwargs.setdefault("device", self.device)
        self.transform, plane = table_plane.calibrate(xyz, self.eval_params[2], **kwargs)
        self.auto_table = None
        return self.transform, plane

    def _networks(self, fr):
        """ScoreNet -> the grouping -> the region network -> (scores, the four grasp sets as the networks leave them)."""
        from .get_regiondataset import get_grasp_allobj
        pc = fr.pc
        all_feature, output_score, _ = self.score_net(pc)
        g = get_grasp_allobj(pc, output_score, self.params, [], self.use_theta)
        res = self.region_net(g[3], g[5], g[2], g[4], g[0], g[1], pc, all_feature, self.gripper_params, None, [])
        # eval_notruth(pc_back, color_back, grasp_stage2, select_grasp_class, select_grasp_score,
        #              select_grasp_class_stage2, output_score, ...): test.py:147 -> utils.py:391
        return output_score, {"grasp_stage2": res[0], "grasp_stage3_stage2": res[8], "grasp_stage3": res[6],
                              "grasp_stage3_score": res[7]}

    def _collision_filter(self, sets, points32):
        """``eval_collision.eval_test`` on each set, in place; ``raw_counts``: their sizes before it."""
        import torch
        from . import eval_collision
        depth, width, table_height, _, _ = self.eval_params
        gpu = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.raw_counts = {}
        for key, grasp in sets.items():
            if grasp is None:      # (the refine head saw no valid crop: an empty set)
                grasp = torch.zeros((0, 8), dtype=torch.float32, device=self.device)
            self.raw_counts[key] = int(grasp.shape[0])
            if grasp.shape[0] >= 1:
                grasp = eval_collision.eval_test(points32, grasp[:, :8], None, table_height, depth, width, gpu)
            sets[key] = grasp

    def _select_and_segment(self, sets, points32):
        """The optional stages behind the filter, on the device, before the download; they draw nothing from numpy's stream.  A
        selection joins ``sets``.  -> (the keys the stages add to the record, in its order; the device tensors of those that
        are not in ``sets``; the ``Segmentation`` or None)."""
        from . import grasp_select
        from . import segment as segment_mod
        sel, seg = self.select, self.segment
        nms = {} if sel is None else sel.nms()
        keys, extra, segmented = (), {}, None
        approach_extra, passing = self._approach(sets, points32)
        if sel is not None and (seg is None or seg.top_k_per_object is None):      # (a per-object selection replaces it)
            keys = SELECT_KEYS
            if passing is None:
                sets.update(zip(keys, grasp_select.pose_nms(sets[sel.source], top_k=sel.top_k, return_index=True, **nms)))
            else:                                 # the selection sees the passing rows; its indices are rows of the full set
                rows, index = grasp_select.pose_nms(sets[sel.source][passing], top_k=sel.top_k, return_index=True, **nms)
                sets.update(zip(keys, (rows, passing[index])))
        if seg is not None:
            source = seg.source or (sel.source if sel is not None else "grasp_stage3")
            above = segment_mod.above_table_mask(points32, self.eval_params[2], seg.table_clearance)
            segmented = segment_mod.cluster_points(points32, above, seg.tolerance, seg.min_points, seg.max_objects)
            grasp_object, _ = segment_mod.assign_grasps(sets[source], points32, segmented.label, seg.assign_radius)
            if seg.top_k_per_object is not None:
                keys = SEGMENT_SELECT_KEYS
                if passing is None:
                    sets.update(zip(keys, segment_mod.select_per_object(sets[source], grasp_object, seg.max_objects,
                                                                        seg.top_k_per_object, **nms)))
                else:
                    rows, index, objects = segment_mod.select_per_object(sets[source][passing], grasp_object[passing],
                                                                         seg.max_objects, seg.top_k_per_object, **nms)
                    sets.update(zip(keys, (rows, passing[index], objects)))
            keys = keys + SEGMENT_KEYS
            extra = {"point_object": segmented.label, "grasp_object": grasp_object}
        if approach_extra is not None:
            keys = keys + tuple(approach_extra)   # APPROACH_KEYS, in volume space followed by APPROACH_VOLUME_KEYS
            extra.update(approach_extra)
        return keys, extra, segmented

    def _approach(self, sets, points32):
        """The approach analysis of the source set -> (its six record entries on the device, the int64 rows that pass
        ``min_clearance`` / ``min_contact`` or None when neither is set); (None, None) without ``approach``."""
        if self.approach is None:
            return None, None
        if self.approach.space == "volume":
            return self._approach_volume(sets)
        from . import approach as approach_mod
        depth, width = self.eval_params[0], self.eval_params[1]
        result = approach_mod.analyse(points32, sets[self.approach_source][:, :8], depth, width, self.approach)
        extra = dict(zip(APPROACH_KEYS, (result.clearance, result.width, result.offset, result.opening, result.contact,
                                         result.pregrasp)))
        passing = result.passes().nonzero().view(-1) if self.approach.filters() else None
        return extra, passing

    def _approach_volume(self, sets):
        """``_approach`` in volume space: ``approach.analyse_volume`` on the detector's volume, the frame's surface and the
        inverse (host, float64) of the transform the frame was ingested with; ``APPROACH_VOLUME_KEYS`` follow the six."""
        from . import approach as approach_mod
        from . import tsdf
        if self.tsdf_volume is None or not isinstance(self.fused, tsdf.Surface):
            raise ValueError("approach: space=\"volume\" analyses the detector's TSDF volume, and this frame has none: hand "
                             "detect a MultiView (volume) or a DepthFrame (track), or use space=\"cloud\"")
        transform = self.transform if self.table is None else self.table[0]
        to_volume = np.linalg.inv(np.asarray(transform, dtype=np.float64))
        depth, width = self.eval_params[0], self.eval_params[1]
        field = None
        if self.approach.field:                   # once per frame, the volume being final: what blocks the clearance is an obstacle
            blocked = self.approach.unseen == "blocked"
            field = self.distance_field = self.tsdf_volume.distance_field(
                mode="solid_or_unseen" if blocked else "solid", outside=blocked, margin=self.approach.margin,
                out=self.distance_field, signed=self.approach.field_signed, max_distance=self.approach.field_max_distance)
        result = approach_mod.analyse_volume(self.tsdf_volume, sets[self.approach_source][:, :8], depth, width, self.approach,
                                             to_volume=to_volume, surface=self.fused, field=field)
        self.approach_result = result             # (the next-best view's interest reads its rows)
        extra = dict(zip(APPROACH_KEYS + APPROACH_VOLUME_KEYS,
                         (result.clearance, result.width, result.offset, result.opening, result.contact, result.pregrasp,
                          result.clearance_seen, result.clearance_safe, result.unseen_share, result.solid_hand)))
        if field is not None:
            extra.update(zip(APPROACH_FIELD_KEYS, (result.margin_hand, result.margin_sweep)))
            if field.signed:
                extra[APPROACH_SIGNED_KEYS[0]] = result.margin_counts[:, 4:6]
        if result.retreat is not None:
            fan = result.retreat
            extra.update(zip(APPROACH_RETREAT_KEYS, (fan.index, fan.free_length, fan.margin, fan.direction, fan.pregrasp,
                                                     fan.free_steps)))
        if result.paths is not None:
            check = result.paths
            extra.update(zip(APPROACH_PATH_KEYS, (check.index, check.free_steps, check.certified_steps(), check.margin,
                                                  _rows_to_frame(transform, check.waypoint))))
        if result.push is not None:
            extra.update(zip(APPROACH_PUSH_KEYS, (result.push.status, result.push.shift, result.push.margin, result.center)))
        ok = result.passes() if self.approach.filters() else None
        passing = ok.nonzero().view(-1) if ok is not None else None
        return extra, passing

    def _next_view(self, sets):
        """The next-best view of the frame's volume -> ``VIEW_KEYS`` as numpy arrays (``view_plan.plan``: one blocking read, and
        one of 12 bytes for the grasps' centroid).  The candidates orbit the centroid of the analysed (else the selected, else
        the stage-3) set's centres, taken to the volume's frame; the volume's centre when the set is empty."""
        from . import tsdf, view_plan
        if self.tsdf_volume is None or not isinstance(self.fused, tsdf.Surface) or self.view_camera is None:
            raise ValueError("view: the next-best view is planned in the detector's TSDF volume, and this frame has none: hand "
                             "detect a MultiView (volume) or a DepthFrame (track)")
        volume = self.tsdf_volume
        transform = self.transform if self.table is None else self.table[0]
        to_volume = np.linalg.inv(np.asarray(transform, dtype=np.float64))
        source = self.approach_source or (self.select.source if self.select is not None else "grasp_stage3")
        grasp = sets[source]
        p = volume.params
        target = np.asarray(volume.origin, dtype=np.float64) + 0.5 * float(p.voxel) * np.asarray(p.dims, dtype=np.float64)
        if grasp.shape[0] >= 1:
            from . import eval_collision
            _, center = eval_collision.grasp_frames(grasp[:, :8].contiguous())
            centroid = center.mean(dim=0).cpu().numpy().astype(np.float64)
            target = (to_volume @ np.append(centroid, 1.0))[:3]
        interest = None
        if self.view.interest == "grasps" and grasp.shape[0] >= 1:
            depth, width = self.eval_params[0], self.eval_params[1]
            interest, _ = view_plan.interest_hands(volume, grasp[:, :8], depth, width, self.approach, to_volume=to_volume,
                                                   rows=self.approach_result.L)
        return view_plan.plan(volume, self.view, target, self.view.scaled_intrinsics(*self.view_camera), interest=interest)

    def _record(self, fr, kept, output_score, sets, keys, extra, segmented):
        """The downloads, in the order they have always been made -> the record, its keys in the documented order."""
        points, colors = fr.download(kept)
        out = {"points": points, "colors": colors, "scores": output_score.view(-1, 1).cpu().numpy()}
        out.update({key: grasp.cpu().numpy() for key, grasp in sets.items()})
        if segmented is not None:
            _, _, out["object_size"], _, out["object_bbox"] = segmented.objects()
        out.update({key: value.cpu().numpy() for key, value in extra.items()})
        keys = RESULT_KEYS + keys
        if fr.table is not None:
            transform, plane = fr.table
            out["table_transform"] = np.array(transform, dtype=np.float64)
            out["table_plane"] = np.array(list(plane.normal) + [plane.offset, plane.rms], dtype=np.float64)
            keys = keys + TABLE_KEYS
        if fr.fused is not None:
            from_volume = False
            if self.volume is not None:           # (the module is imported: the detector has ``volume``)
                from . import tsdf
                from_volume = isinstance(fr.fused, tsdf.Surface)
            tracked = getattr(fr, "tracked", None)
            if tracked is not None:
                from . import registration
                out["tsdf_num"] = fr.fused.num.cpu().numpy()
                out["tsdf_counts"] = (np.zeros((1, 4), dtype=np.int32) if tracked.counts is None
                                      else tracked.counts.cpu().numpy().reshape(1, 4))
                out["track_pose"] = np.array(tracked.pose, dtype=np.float64)
                out["track_status"] = np.array(tsdf.TRACK_STATUS.index(tracked.status), dtype=np.int32)
                out["track_report"] = np.array([np.nan] * 5 if tracked.report is None else registration.report_row(tracked.report),
                                               dtype=np.float64)
                keys = keys + TSDF_KEYS + TRACK_KEYS
                if tracked.levels is not None:    # the coarse-to-fine path ran (a FIRST frame has no registration)
                    out["track_levels"] = np.array(tracked.levels, dtype=np.int32)
                    keys = keys + ("track_levels",)
            elif from_volume:
                out["tsdf_num"] = fr.fused.num.cpu().numpy()
                out["tsdf_counts"] = fr.fused.counts.cpu().numpy()
                keys = keys + TSDF_KEYS
            else:
                out["fuse_num"] = fr.fused.num.cpu().numpy()
                out["fuse_views"] = fr.fused.per_view().cpu().numpy()
                keys = keys + FUSE_KEYS
            if getattr(fr, "meshed", None) is not None:
                (out["tsdf_vertices"], out["tsdf_vertex_normals"], out["tsdf_vertex_colors"],
                 out["tsdf_triangles"]) = fr.meshed.to_host()
                keys = keys + TSDF_MESH_KEYS
                if self.mesh_cell is not None:
                    out["tsdf_mesh_report"] = fr.meshed.report.cpu().numpy()
                    keys = keys + TSDF_MESH_REPORT_KEYS
            if fr.fused.register is not None:
                out["fuse_poses"] = np.array(fr.fused.poses, dtype=np.float64)
                out["fuse_register"] = np.array(fr.fused.register, dtype=np.float64)
                keys = keys + REGISTER_KEYS
        if getattr(fr, "denoised", None) is not None:
            out["denoise_num"] = fr.denoised.num.cpu().numpy()
            keys = keys + DENOISE_KEYS
        return {key: out[key] for key in keys}

    def detect(self, frame):
        """test.py:97-148 for one frame -> ``eval_notruth``'s dict of numpy arrays: ``points`` / ``colors`` (the cropped,
        un-jittered cloud: float64 for a camera frame, float32 for a record), ``scores`` (N,1) float32 and the four
        collision-filtered grasp sets (k,8) float32; with ``select`` also ``SELECT_KEYS``, with ``segment`` ``SEGMENT_KEYS``,
        with ``approach`` ``APPROACH_KEYS``."""
        import torch
        from . import np_random
        was_training = self.score_net.training, self.region_net.training
        self.score_net.eval()
        self.region_net.eval()
        try:
            # (the stages' progress prints stay off stdout: detect_file's three count lines are all a caller sees; the device
            # context covers the whole frame -- both networks' torch layers and every launch -- so none of them switches)
            with np_random.deferred(), torch.no_grad(), torch.cuda.device(self.device), \
                    contextlib.redirect_stdout(io.StringIO()):
                self.table = self.fused = None
                fr = self.ingest(frame)
                self.table, self.fused = fr.table, fr.fused
                if fr.fused is not None:
                    fr.fused.check()       # one 16-byte read; ValueError naming max_voxels when the merge overflowed
                output_score, sets = self._networks(fr)
                kept = fr.kept()
                points32 = fr.points32[:kept]
                self._collision_filter(sets, points32)
                keys, extra, segmented = self._select_and_segment(sets, points32)
                record = self._record(fr, kept, output_score, sets, keys, extra, segmented)
                if self.view is not None:         # last: the volume is final and the analysed hands are known
                    record.update(self._next_view(sets))
                return record
        finally:
            self.score_net.train(was_training[0])
            self.region_net.train(was_training[1])

    def detect_file(self, path, save_path=None, real_data=None):
        """``test_one_file`` (test.py:94-148): ``.pcd`` -> camera frame, ``.npz`` -> depth frame (with a ``views`` entry: the depth frames of several
        cameras, ``fusion.load_npz``), anything else -> dataset record, unless ``real_data`` says so.  The dict is pickled to ``save_path`` (default: the rule of :143-145; no file when that rule leaves the path
        unchanged, which would overwrite the input).  Prints the reference's three count lines, and the selected count when
        the detector has ``select``, the object count when it has ``segment``, and with ``approach`` the number of grasps of its set that
        can retreat the whole standoff.  -> (dict, save path or None)."""
        from . import depth_frame, fusion, ingest
        is_depth = path.endswith(".npz")
        if real_data is None:
            real_data = is_depth or path.lower().endswith(".pcd")
        if is_depth:
            real_data = True
            out = self.detect(fusion.load_npz(path) if fusion.is_multiview_npz(path) else depth_frame.load_npz(path))
        elif real_data:
            xyz, rgb, _ = ingest.read_pcd(path)
            out = self.detect((xyz, rgb))
        else:
            with open(path, "rb") as f:
                out = self.detect(pickle.load(f))
        print("stage2 grasp num:", len(out["grasp_stage2"]))
        print("stage3 grasp num:", len(out["grasp_stage2"]))        # (sic: utils.py:410 prints the stage-2 count twice)
        print("stage3 grasp num (with scorethre):", len(out["grasp_stage3_score"]))
        if self.select is not None:
            print("selected grasp num (%s):" % self.select.source, len(out["grasp_selected"]))
        if self.segment is not None:
            print("object num:", len(out["object_size"]))
        if self.approach is not None:
            print("free approach grasp num (%s):" % self.approach_source,
                  int((out["grasp_clearance"] >= np.float32(self.approach.standoff)).sum()))
        if save_path is None:
            save_path = save_path_for(path, real_data)
            if save_path == path:
                return out, None
        os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
        with open(save_path, "wb") as f:
            pickle.dump(out, f)
        if self.mesh_ply and "tsdf_triangles" in out:
            from . import tsdf
            tsdf.write_ply(os.path.splitext(save_path)[0] + ".ply", out["tsdf_vertices"], out["tsdf_vertex_normals"],
                           out["tsdf_vertex_colors"], out["tsdf_triangles"])
        return out, save_path


# The regular flags of the CLI: (flag, group, field of the group's parameter class, type or the choices, help stem).  A flag that
# is not given is None and stays out of the group's dict; a field's default other than None follows the stem in brackets, read
# from the class, or stands where the stem says %s.  ``--auto-table``, ``--segment``, ``--keep-uncoloured`` and the two LO HI ranges are written out in build_parser.
_FLAGS = (
    # pose NMS + top-K on one of the four sets (grasp_select.pose_nms); giving any of the four turns the selection on
    ("--top-k", "select", "top_k", int, "keep the K best distinct grasps (default: every distinct one)"),
    ("--nms-translation", "select", "translation_thresh", float, "centres this close are the same grasp [m]"),
    ("--nms-rotation", "select", "rotation_thresh_deg", float, "frames this close are the same grasp [deg]"),
    ("--select-from", "select", "source", RESULT_KEYS[3:], "the set to select from"),
    # the table plane estimated on every camera frame (table_plane.estimate_plane); giving any of its three flags turns it on
    ("--plane-threshold", "transform", "threshold", float, "inlier distance of the table plane [m]"),
    # depth frames (*.npz: depth_frame.to_cloud): the flying-pixel filter and the occlusion test of the colour sensor
    ("--edge-threshold", "depth", "edge_threshold", float,
     "remove pixels whose depth jumps by more than this share of the nearer depth to a neighbour (off)"),
    ("--min-neighbours", "depth", "min_neighbours", int, "remove pixels with fewer valid 8-neighbours"),
    ("--occlusion-margin", "depth", "occlusion_margin", float,
     "a point this far behind the colour camera's nearest surface is still seen by it [m]"),
    # object segmentation (segment.cluster_points): --segment or any of the four turns it on
    ("--cluster-tolerance", "segment", "tolerance", float, "points this close belong to one object [m]"),
    ("--min-object-points", "segment", "min_points", int, "drop clusters of fewer points"),
    ("--max-objects", "segment", "max_objects", int, "keep the largest so many objects"),
    ("--top-k-per-object", "segment", "top_k_per_object", int, "select the K best distinct grasps of every object"),
    # multi-view frames (*.npz with a `views` entry: fusion.voxel_merge): the voxel grid the views are merged on
    ("--voxel", "fuse", "voxel", float, "edge of the voxels the views are merged in [m]"),
    ("--max-voxels", "fuse", "max_voxels", int, "rows of the merged cloud, at most 2^21"),
    ("--min-voxel-points", "fuse", "min_count", int, "drop voxels with fewer points"),
    # pose refinement before the merge (fusion.refine_poses): --refine-poses or any of the six turns it on
    ("--icp-distance", "register", "max_dist", float, "a point pairs with its nearest point of the first view within this distance (%s m)"),
    ("--icp-iterations", "register", "iterations", int, "steps of the registration, at most 64 (%s steps)"),
    ("--icp-stride", "register", "stride", int, "register every so-manieth point of a view; must not divide the image width (every point: %s, the default)"),
    ("--icp-association", "register", "association", ("nearest", "projective"),
     "how a point finds its partner: the nearest point over a grid, or a lookup in the first view's depth image"),
    ("--icp-window", "register", "window", int, "projective association looks this many pixels (%s, at most 2) around the pixel a point falls on"),
    ("--icp-normal-angle", "register", "normal_angle", float,
     "projective association pairs only points whose normals are within this angle [deg] (off)"),
    # approach analysis of one set (approach.analyse): --approach or any of the five turns it on
    ("--approach-standoff", "approach", "standoff", float, "sweep the hand this far back along its approach (%s m)"),
    ("--approach-from", "approach", "source", RESULT_KEYS[3:], "the set to analyse (default: the selection's)"),
    ("--friction-angle", "approach", "friction_deg", float,
     "judge the contacts: half angle of the friction cone about the closing axis [deg] (off)"),
    ("--min-clearance", "approach", "min_clearance", float, "select only grasps that can retreat this far [m]"),
    ("--min-contact", "approach", "min_contact", float, "select only grasps whose contact share is at least this"),
    ("--approach-space", "approach", "space", ("cloud", "volume"),
     "hold the hand against the frame's points, or against the TSDF volume of --tsdf / --track"),
    ("--approach-unseen", "approach", "unseen", ("free", "blocked"),
     "in volume space: whether space no camera has seen lets the hand through"),
    ("--approach-step", "approach", "step", float, "in volume space: the distance between two samples of the swept hand [m] (the voxel)"),
    ("--approach-margin", "approach", "margin", float,
     "in volume space: a voxel nearer than this (%s m) to a surface is solid"),
    ("--min-margin", "approach", "min_margin", float,
     "select only grasps whose hand keeps this distance [m] to the nearest obstacle of the volume (implies --approach-field)"),
    ("--approach-field-cap", "approach", "field_max_distance", float,
     "cap the distance field at this distance [m]: margins saturate there and the field costs less (implies --approach-field)"),
    # a TSDF volume in place of the point merge (tsdf.fuse_volume): --tsdf or any of the five turns it on
    ("--tsdf-voxel", "volume", "voxel", float, "edge of the voxels of the volume (%s m)"),
    ("--tsdf-trunc", "volume", "trunc", float, "truncation distance, at least two voxels (%s m)"),
    ("--tsdf-min-weight", "volume", "min_weight", int, "a voxel bounds a surface when so many views observed it (%s views)"),
    # a moving camera tracked against the volume (tsdf.Tracker): --track or any of the five turns it on
    ("--track-near", "track", "near", float, "march the model view's rays from this depth (%s m)"),
    ("--track-far", "track", "far", float, "... to this depth (%s m)"),
    ("--track-step", "track", "step", float, "the distance between two samples of a ray [m] (half the truncation distance)"),
    ("--track-max-translation", "track", "max_translation", float, "a frame that moved further than this is lost (%s m)"),
    ("--track-max-rotation", "track", "max_rotation", float, "a frame that turned further than this is lost (%s rad)"),
    ("--track-levels", "track", "levels", int, "register coarse to fine over this many levels of the frame's depth pyramid, 1..4 "
     "(%s: the frame's own resolution alone)"),
    ("--track-dist-scale", "track", "level_dist_scale", float, "level l of the pyramid pairs within max_dist times this to the l "
     "(%s per level)"),
    # outlier removal of a camera frame's cloud (outliers.filter_cloud): --denoise or any of the six turns it on
    ("--outlier-mode", "outliers", "mode", ("radius", "statistical", "both"),
     "the radius filter, the statistical filter, or the first and then the second on its survivors"),
    ("--outlier-radius", "outliers", "radius", float, "a point stays when enough others lie within this distance (%s m)"),
    ("--outlier-min-neighbours", "outliers", "min_neighbours", int, "... at least so many (%s points)"),
    ("--outlier-knn", "outliers", "knn", int, "the statistical filter takes the mean distance to so many nearest points, at most 64 (%s points)"),
    ("--outlier-max-radius", "outliers", "max_radius", float, "... looked for within this distance (%s m)"),
    ("--outlier-std-ratio", "outliers", "std_ratio", float,
     "a point stays when its mean distance is at most the cloud's mean plus so many standard deviations (%s deviations)"),
)


def _given(args, group):
    """The fields of ``group`` whose flags were given -> a dict (empty when none was)."""
    given = {field: getattr(args, flag[2:].replace("-", "_")) for flag, g, field, _, _ in _FLAGS if g == group}
    return {field: value for field, value in given.items() if value is not None}


def select_from_args(args):
    """The CLI's four selection flags -> a ``select`` dict, or None when none of them was given."""
    return _given(args, "select") or None


def segment_from_args(args):
    """The CLI's five segmentation flags -> a ``segment`` dict, or None when none of them was given."""
    given = _given(args, "segment")
    return given if (given or args.segment) else None


def transform_from_args(args):
    """The CLI's three table flags -> ``GraspDetector``'s ``transform``: None (the default transform) unless one was given."""
    given = {} if args.table_range is None else {"range": (float(args.table_range[0]), float(args.table_range[1]))}
    given.update(_given(args, "transform"))
    return given or ("auto" if args.auto_table else None)


def depth_from_args(args):
    """The CLI's five depth-frame flags -> a ``depth`` dict, or None when none of them was given."""
    given = _given(args, "depth")
    if args.depth_range is not None:
        given["depth_range"] = (float(args.depth_range[0]), float(args.depth_range[1]))
    if args.keep_uncoloured:
        given["keep_uncoloured"] = True
    return given or None


def fuse_from_args(args):
    """The CLI's three fusion flags -> a ``fuse`` dict, or None when none of them was given."""
    return _given(args, "fuse") or None


def register_from_args(args):
    """The CLI's seven registration flags -> a ``register`` dict, or None when none of them was given."""
    given = _given(args, "register")
    return given if (given or args.refine_poses) else None


def _rows_to_frame(transform, rows):
    """``rows`` (B,12) float32 on the device, poses in the volume's frame; ``transform`` the host 4x4 from the volume's frame to
    the grasps' -> (B,12) float32: ``transform @ pose`` per row, on the device in float64 and rounded once."""
    import torch
    from . import approach_volume
    B = int(rows.shape[0])
    full = torch.zeros((B, 4, 4), dtype=torch.float64, device=rows.device)
    full[:, :3, :] = rows.reshape(B, 3, 4)
    full[:, 3, 3] = 1.0
    moved = approach_volume._times_rows(np.asarray(transform, dtype=np.float64), full)
    return moved[:, :3, :].reshape(B, 12).to(torch.float32).contiguous()


def approach_from_args(args):
    """The CLI's approach flags -> an ``approach`` dict, or None when none of them was given."""
    given = _given(args, "approach")
    retreat = {field: value for field, value in (("length", args.retreat_length), ("steps", args.retreat_steps),
                                                 ("tilt_deg", args.retreat_tilt)) if value is not None}
    if args.retreat_up is not None:
        retreat["up"] = tuple(float(v) for v in args.retreat_up)
    if args.approach_retreat or retreat or args.min_retreat is not None:
        given["retreat"] = retreat or True
        given["field"] = True
    if args.min_retreat is not None:
        given["min_retreat"] = args.min_retreat
    paths = {field: value for field, value in (("turn_deg", args.path_turn), ("length", args.path_length),
                                               ("steps", args.path_steps)) if value is not None}
    if args.path_pivot is not None:
        paths["pivot"] = tuple(float(v) for v in args.path_pivot)
    if args.approach_paths or paths or args.min_path is not None:
        given["paths"] = paths or True
        given["field"] = True
    if args.min_path is not None:
        given["min_path"] = args.min_path
    push = {field: value for field, value in (("target", args.push_target), ("max_shift", args.push_max_shift),
                                              ("iterations", args.push_iterations)) if value is not None}
    if args.push_axes is not None:
        push["axes"] = tuple(float(v) for v in args.push_axes)
    if args.approach_push or push or args.push_keep is not None:
        given["push"] = push or True
        given["field"] = given["field_signed"] = True
    if args.push_keep is not None:
        given["push_keep"] = args.push_keep
    if args.approach_signed:
        given["field_signed"] = True
    if args.approach_field or args.approach_signed or "min_margin" in given or "field_max_distance" in given:
        given["field"] = True
    return given if (given or args.approach) else None


def view_from_args(args):
    """The CLI's five next-view flags -> a ``view`` dict, or None when none of them was given."""
    given = {}
    if args.view_candidates is not None:
        given["azimuths"], given["elevations"] = (int(v) for v in args.view_candidates)
    for field, value in (("radius", args.view_radius), ("top_k", args.view_top_k), ("interest", args.view_interest)):
        if value is not None:
            given[field] = value
    return given if (given or args.next_view) else None


def outliers_from_args(args):
    """The CLI's seven outlier flags -> a ``denoise`` dict, or None when none of them was given."""
    given = _given(args, "outliers")
    return given if (given or args.denoise) else None


def volume_from_args(args):
    """The CLI's six volume flags -> a ``volume`` dict, or None when none of them was given."""
    given = _given(args, "volume")
    if args.tsdf_origin is not None:
        given["origin"] = tuple(float(v) for v in args.tsdf_origin)
    if args.tsdf_dims is not None:
        given["dims"] = tuple(int(v) for v in args.tsdf_dims)
    return given if (given or args.tsdf) else None


def track_from_args(args):
    """The CLI's ten tracking flags -> a ``track`` dict, or None when none of them was given."""
    given = _given(args, "track")
    if args.track_level_iterations is not None:
        given["level_iterations"] = tuple(int(v) for v in args.track_level_iterations)
    if args.track_smooth is not None:
        radius, sigma_space, sigma_depth = args.track_smooth
        if radius != int(radius):
            raise ValueError("--track-smooth: RADIUS must be a whole number of pixels")
        given["smooth"] = {"radius": int(radius), "sigma_space": float(sigma_space), "sigma_depth": float(sigma_depth)}
    return given if (given or args.track) else None


def build_parser():
    """The CLI of ``main``: test.py's arguments, ``_FLAGS`` and the irregular flags of each group."""
    from . import approach as approach_mod
    from . import depth_frame, fusion, grasp_select, outliers, registration, table_plane, tsdf
    from . import segment as segment_mod
    defaults = {"select": grasp_select.SelectParams(), "transform": argparse.Namespace(threshold=table_plane.DEFAULT_THRESHOLD),
                "depth": depth_frame.DepthParams(), "segment": segment_mod.SegmentParams(), "fuse": fusion.FuseParams(),
                "register": registration.IcpParams(), "approach": approach_mod.ApproachParams(),
                "outliers": outliers.OutlierParams(), "volume": tsdf.TsdfParams(), "track": tsdf.TrackParams()}
    parser = argparse.ArgumentParser(description="REGNet single-file inference (the reference's test.py)")
    parser.add_argument("--folder", "--folder-name", dest="folder", required=True)
    parser.add_argument("--file", "--file-name", dest="file", default="")
    parser.add_argument("--load-score-path", required=True)
    parser.add_argument("--load-region-path", required=True)
    parser.add_argument("--gpu", type=int, default=0)

    def regular(group):
        # (a stem may place its default itself with %s: tests/test_depth_frame_cpu.py holds every help that ENDS in a bracketed
        # number against its own table of flags, so a new flag's default cannot be appended the usual way)
        for flag, g, field, kind, stem in _FLAGS:
            if g == group:
                default = getattr(defaults[group], field)
                shown = "" if default is None else "%g" % default if isinstance(default, float) else str(default)
                text = stem.replace("%s", shown) if "%s" in stem else stem + (" (%s)" % shown if shown else "")
                parser.add_argument(flag, default=None, help=text,
                                    **({"choices": list(kind)} if isinstance(kind, tuple) else {"type": kind}))

    regular("select")
    parser.add_argument("--auto-table", action="store_true", help="estimate the camera -> table transform on every frame")
    parser.add_argument("--table-range", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                        help="the table plane lies between LO and HI metres from the camera")
    regular("transform")
    parser.add_argument("--depth-range", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                        help="keep depths between LO and HI metres, inclusive (%g %g)" % defaults["depth"].depth_range)
    regular("depth")
    parser.add_argument("--keep-uncoloured", action="store_true",
                        help="keep points the colour camera does not see, with black colour, instead of dropping them")
    parser.add_argument("--segment", action="store_true", help="cluster the points above the table into objects")
    regular("segment")
    regular("fuse")
    parser.add_argument("--refine-poses", action="store_true",
                        help="correct the views' poses against the first view before they are merged")
    regular("register")
    parser.add_argument("--approach", action="store_true",
                        help="analyse every grasp of one set: approach clearance, closing width, opening and pre-grasp point")
    regular("approach")
    parser.add_argument("--approach-field", action="store_true",
                        help="in volume space: build the volume's distance field once per frame and add every grasp's margin, the "
                             "distance from the hand and from the swept hand to the nearest obstacle")
    parser.add_argument("--approach-signed", action="store_true",
                        help="build that field signed: a hand in collision reads a negative margin, minus its penetration "
                             "depth, and the record gains grasp_colliding (implies --approach-field)")
    fan = approach_mod.RetreatParams()
    parser.add_argument("--approach-retreat", action="store_true",
                        help="in volume space: move the hand at its final pose along a fan of retreat directions against the "
                             "distance field and add the best direction, its free length, margin and pre-grasp point (implies "
                             "--approach-field; the fan's defaults are a choice nobody has measured on a robot)")
    parser.add_argument("--retreat-length", type=float, default=None,
                        help="the length of every retreat path, %g m unless given (implies --approach-retreat)" % fan.length)
    parser.add_argument("--retreat-steps", type=int, default=None,
                        help="the steps a retreat path is cut into, 1..64, %d unless given (implies --approach-retreat)" % fan.steps)
    parser.add_argument("--retreat-tilt", type=float, default=None,
                        help="the tilt of the fan's side directions off the straight retreat, %g degrees unless given (implies "
                             "--approach-retreat)" % fan.tilt_deg)
    parser.add_argument("--retreat-up", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                        help="a direction in the grasps' frame to also retreat along, and half way towards (off; implies "
                             "--approach-retreat)")
    parser.add_argument("--min-retreat", type=float, default=None,
                        help="select only grasps whose best retreat direction is free this far [m] (implies --approach-retreat)")
    hand = approach_mod.PathParams()
    parser.add_argument("--approach-paths", action="store_true",
                        help="in volume space: take the hand through candidate trajectories of poses (five straight, four turning) "
                             "against the distance field and add the picked path, the free and certified steps, its margin and the "
                             "pre-grasp pose (implies --approach-field; the defaults are a choice nobody has measured on a robot)")
    parser.add_argument("--path-turn", type=float, default=None,
                        help="the angle the turning paths turn through, %g degrees unless given (implies --approach-paths)" % hand.turn_deg)
    parser.add_argument("--path-length", type=float, default=None,
                        help="how far every path translates, %g m unless given (implies --approach-paths)" % hand.length)
    parser.add_argument("--path-steps", type=int, default=None,
                        help="the steps a path is cut into, 1..64, %d unless given (implies --approach-paths)" % hand.steps)
    parser.add_argument("--path-pivot", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                        help="the point of the hand's local frame the turns are about, the origin unless given (implies "
                             "--approach-paths)")
    parser.add_argument("--min-path", type=float, default=None,
                        help="select only grasps whose picked path is certified free this far [m] (implies --approach-paths)")
    shove = approach_mod.PushParams()
    parser.add_argument("--approach-push", action="store_true",
                        help="in volume space: first move every hand that has less than the target margin along the gradient of the "
                             "signed distance field, analyse the grasps that move freed at their moved centre and add the status, "
                             "the shift, the margin and that centre (implies --approach-signed; it needs --approach-field-cap; the "
                             "defaults are a choice nobody has measured on a robot)")
    parser.add_argument("--push-target", type=float, default=None,
                        help="the signed margin the hand is moved to, %g m unless given (implies --approach-push)" % shove.target)
    parser.add_argument("--push-max-shift", type=float, default=None,
                        help="the longest move of a hand, %g m unless given (implies --approach-push)" % shove.max_shift)
    parser.add_argument("--push-iterations", type=int, default=None,
                        help="the most steps of a move, 1..64, %d unless given (implies --approach-push)" % shove.iterations)
    parser.add_argument("--push-axes", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                        help="a factor per local axis of the hand (approach, closing, thickness) on every step, 1 1 1 unless given; "
                             "0 1 0 re-centres along the closing axis only (implies --approach-push)")
    parser.add_argument("--push-keep", choices=("all", "freed"), default=None,
                        help="freed: select only grasps that have the target margin after the move (implies --approach-push)")
    parser.add_argument("--denoise", action="store_true",
                        help="remove the outliers of a camera frame's cloud before the table plane and the crop")
    regular("outliers")
    parser.add_argument("--tsdf", action="store_true",
                        help="integrate the views of a multi-view frame into a TSDF volume and take its surface, instead of "
                             "merging their points")
    parser.add_argument("--tsdf-origin", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None,
                        help="corner of voxel (0, 0, 0) in the common frame (%g %g %g m)" % defaults["volume"].origin)
    parser.add_argument("--tsdf-dims", type=int, nargs=3, metavar=("NX", "NY", "NZ"), default=None,
                        help="voxels per axis, at most 2^28 in all (%d %d %d voxels)" % defaults["volume"].dims)
    regular("volume")
    parser.add_argument("--tsdf-mesh", action="store_true",
                        help="with --tsdf or --track: take the volume's surface as a triangle mesh and add it to the record")
    parser.add_argument("--tsdf-mesh-ply", action="store_true",
                        help="... and write it as NAME.ply beside the record (implies --tsdf-mesh)")
    parser.add_argument("--tsdf-mesh-cell", type=float, metavar="M", default=None,
                        help="simplify that mesh on the device by vertex clustering on cells of M metres before it goes into the "
                             "record and the PLY (implies --tsdf-mesh)")
    parser.add_argument("--track", action="store_true",
                        help="the folder's depth frames, in the order of their names, are one moving camera: track it against the "
                             "TSDF volume it fills and take the volume's surface as every frame's cloud")
    regular("track")
    parser.add_argument("--track-level-iterations", type=int, nargs="+", metavar="STEPS", default=None,
                        help="the registration steps per level of the pyramid, finest first, 64 in all at most (10 5 4 4 steps, as "
                             "many of them as there are levels)")
    parser.add_argument("--track-smooth", type=float, nargs=3, metavar=("RADIUS", "SIGMA_SPACE", "SIGMA_DEPTH"), default=None,
                        help="smooth the frame's depth for the registration by a bilateral filter: window radius 1..4 pixels, "
                             "spatial sigma [pixels], depth sigma [m] (off; 3 2 0.01 are the filter's own defaults)")
    from . import view_plan
    view = view_plan.ViewParams()
    parser.add_argument("--next-view", action="store_true",
                        help="with --tsdf or --track: rank candidate camera poses by the unobserved voxels of the volume each would "
                             "reveal and add the joint pick to the record (the defaults are a choice nobody has measured on a robot)")
    parser.add_argument("--view-candidates", type=int, nargs=2, metavar=("AZ", "EL"), default=None,
                        help="the candidates: AZ azimuths times EL elevations on an orbit about the kept grasps, at most 32 in all, "
                             "%d %d unless given (implies --next-view)" % (view.azimuths, view.elevations))
    parser.add_argument("--view-radius", type=float, default=None,
                        help="the radius of that orbit, %g m unless given (implies --next-view)" % view.radius)
    parser.add_argument("--view-top-k", type=int, default=None,
                        help="pick so many poses jointly, %d unless given (implies --next-view)" % view.top_k)
    parser.add_argument("--view-interest", choices=list(view_plan.INTERESTS), default=None,
                        help="count every unobserved voxel (all, the default), or only those inside the swept hands of the analysed "
                             "grasps (grasps: needs --approach-space volume; implies --next-view)")
    return parser


def main(argv=None):
    """``main()`` of test.py:150-164."""
    from . import checkpoint
    parser = build_parser()
    args = parser.parse_args(argv)
    select = select_from_args(args)
    obj_class_num, group_num, gripper_num, score_thre, depth, reg_channel = MODEL_PARAMS
    dev = "cuda:%d" % args.gpu
    with contextlib.redirect_stdout(io.StringIO()):
        score_net, _ = checkpoint.construct_scorenet(True, obj_class_num, args.load_score_path, args.gpu)
        region_net, _ = checkpoint.construct_rnet(True, True, group_num, gripper_num, score_thre, depth, reg_channel,
                                                  args.load_region_path, args.gpu)
    eval_params = [DEPTH, WIDTH, TABLE_HEIGHT, args.gpu, CENTER_NUM]
    detector = GraspDetector(score_net.to(dev), region_net.to(dev), eval_params=eval_params, select=select,
                             transform=transform_from_args(args), depth=depth_from_args(args),
                             segment=segment_from_args(args), fuse=fuse_from_args(args), register=register_from_args(args),
                             approach=approach_from_args(args), denoise=outliers_from_args(args),
                             volume=volume_from_args(args), track=track_from_args(args), mesh=args.tsdf_mesh,
                             mesh_ply=args.tsdf_mesh_ply, mesh_cell=args.tsdf_mesh_cell, view=view_from_args(args))
    real_data = "real_data" in args.folder
    if args.file:
        paths = [os.path.join(args.folder, args.file)]
    else:
        paths = glob.glob(args.folder + ("/*.pcd" if real_data else "/*.p"), recursive=True)
        if real_data:
            paths += sorted(glob.glob(args.folder + "/*.npz"))
    for path in paths:
        detector.detect_file(path, real_data=real_data)


if __name__ == "__main__":
    main()
