"""gmf_amd - MI355X-native GMF multimodal-fusion hot path (PointDSC / DGR plugin surface).

Python host modules with the reference's constructor signatures, ``forward`` signatures and
``state_dict`` keys; all compute goes through libgmf_hip.so (hand-written HIP kernels for gfx950)
over the C ABI declared in include/gmf_hip.h.  There is no CPU or eager-PyTorch fallback.
"""
from .fusion_layer import FusionLayer            # noqa: F401
from .perceiver_io import PerceiverIO            # noqa: F401
from .pointdsc import NonLocalBlock, NonLocalNet, PointDSC, ImageEncoder   # noqa: F401
from .common import rigid_transform_3d, knn      # noqa: F401
from .registration import (weighted_procrustes, weighted_procrustes_batched, GlobalRegistration,  # noqa: F401
                           global_registration_batched, argmin_se3_squared_dist, Transformation, ortho2rotation)
from .matching import nn_match, find_knn_gpu, find_knn_gpu_batch, find_knn_batch, find_pairs    # noqa: F401
from .correspondences import nn_match_mutual, build_correspondences    # noqa: F401
from . import se3 as SE3                         # noqa: F401
from ._lib import check_status, set_handle_per_stream   # noqa: F401
from .solvers import (ransac_correspondence_batched, icp_point_to_point_batched, icp_point_to_plane_batched, RegistrationResult,  # noqa: F401
                      icp_colored_batched, registration_colored_icp,
                      registration_ransac_based_on_correspondence, registration_icp, icp_refine,
                      ransac_feature_matching_batched, registration_ransac_based_on_feature_matching)
from .spectral import spectral_matching_batched, SM   # noqa: F401
from .clique import max_clique_batched, PMC, compatibility_graph   # noqa: F401
from .features import (radius_knn_batched, estimate_normals_batched, compute_fpfh_batched,  # noqa: F401
                       voxel_down_sample_batched, voxel_select_batched, voxel_down_sample, voxel_select, estimate_normals,
                       compute_fpfh_feature, fpfh_descriptors, color_gradients_batched, voxel_down_sample_colored_batched)
from .sparse import (SparsePlan, sparse_conv, sparse_conv_narrow, sparse_conv_narrow_wgrad, sparse_head_l2, ResUNetBN2C,  # noqa: F401
                     ResUNetBN2CX, inlier_coordinates)
from . import fcgf, dgr                          # noqa: F401  (gmf_amd.fcgf.ResUNetBN2C: FCGF; gmf_amd.ResUNetBN2C: the inlier net)
from .dgr import matching_indices_batched, find_correct_correspondence, generate_inlier_input   # noqa: F401
from .multiway import (information_matrix_batched, global_optimization, local_refinement_batched, loop_closure_mask,  # noqa: F401
                       odometry_poses, absolute_trajectory_error, multiway_registration, colored_refinement_batched)
from .fragments import (TsdfMeshes, tsdf_extract_mesh, tsdf_fragment_meshes, tsdf_fragments,      # noqa: F401
                        tsdf_fragments_colored)
from .rgbd import rgbd_pyramids, rgbd_correspondence_map, rgbd_odometry, rgbd_fragments, RGBDPyramids   # noqa: F401
from .losses import ClassificationLoss, SpectralMatchingLoss, TransformationLoss, similarity_matrix   # noqa: F401

__all__ = ["FusionLayer", "PerceiverIO", "NonLocalBlock", "NonLocalNet", "PointDSC", "ImageEncoder",
           "rigid_transform_3d", "knn", "weighted_procrustes", "weighted_procrustes_batched", "GlobalRegistration", "global_registration_batched", "argmin_se3_squared_dist", "Transformation", "ortho2rotation", "nn_match", "nn_match_mutual", "build_correspondences",
           "find_knn_gpu", "SE3", "ClassificationLoss", "SpectralMatchingLoss", "TransformationLoss",
           "similarity_matrix", "check_status", "set_handle_per_stream", "ransac_correspondence_batched",
           "icp_point_to_point_batched", "icp_point_to_plane_batched", "icp_colored_batched", "registration_colored_icp",
           "color_gradients_batched", "voxel_down_sample_colored_batched", "colored_refinement_batched", "RegistrationResult", "registration_ransac_based_on_correspondence", "registration_icp",
           "icp_refine", "radius_knn_batched", "estimate_normals_batched", "compute_fpfh_batched", "voxel_down_sample_batched",
           "voxel_select_batched", "voxel_down_sample", "voxel_select", "estimate_normals", "compute_fpfh_feature",
           "fpfh_descriptors", "SparsePlan", "sparse_conv", "sparse_conv_narrow", "sparse_conv_narrow_wgrad", "sparse_head_l2",
           "ResUNetBN2C", "ResUNetBN2CX",
           "inlier_coordinates", "fcgf", "dgr", "find_knn_gpu_batch", "find_knn_batch", "find_pairs", "matching_indices_batched",
           "find_correct_correspondence", "generate_inlier_input", "ransac_feature_matching_batched",
           "registration_ransac_based_on_feature_matching", "spectral_matching_batched", "SM", "max_clique_batched", "PMC",
           "compatibility_graph", "information_matrix_batched",
           "global_optimization", "local_refinement_batched", "loop_closure_mask", "odometry_poses", "absolute_trajectory_error",
           "multiway_registration", "tsdf_fragments", "tsdf_fragments_colored", "tsdf_fragment_meshes", "tsdf_extract_mesh",
           "TsdfMeshes", "rgbd_pyramids", "rgbd_correspondence_map",
           "rgbd_odometry", "rgbd_fragments", "RGBDPyramids"]
