from .global_volume import TSDFVolume, mesh_from_voxels, render_from_voxels  # noqa: F401
from .mesh_ops import filter_mesh, mesh_components  # noqa: F401
from .mesh_simplify import simplify_mesh  # noqa: F401
from .mesh_decimate import decimate_mesh  # noqa: F401
from .mesh_holes import fill_holes, mesh_boundaries  # noqa: F401
from .mesh_smooth import smooth_mesh, vertex_normals  # noqa: F401
from .mesh_metrics import compare_meshes, face_areas, mesh_distance, sample_mesh  # noqa: F401
from .mesh_align import align_meshes, fit_sim3, transform_mesh  # noqa: F401
from .mesh_raycast import observed_points, render_mesh  # noqa: F401
from .mesh_index import MeshIndex, build_mesh_index  # noqa: F401
from .mesh_texture import (MeshTexture, atlas_classes, atlas_layout, bake_texture, render_mesh_color,  # noqa: F401
                           sized_layout)
from .cloud import (CloudIndex, align_clouds, cloud_distance, cloud_knn, cloud_normals, cloud_outliers,  # noqa: F401
                    compare_clouds, downsample_cloud, filter_cloud, transform_cloud)
from .cloud_cluster import cloud_clusters, cloud_radius_count, filter_cloud_clusters  # noqa: F401
from .cloud_planes import cloud_planes, plane_figures  # noqa: F401
from .cloud_smooth import cloud_mls, smooth_cloud  # noqa: F401
from .cloud_view import observed_cloud_points, render_cloud  # noqa: F401
from .image_metrics import image_metrics  # noqa: F401
from .tsdf_optimizer import TSDFPoseOptimizer  # noqa: F401
from .global_manager import TSDFGlobalIntegrator, TSDFGlobalManager  # noqa: F401
