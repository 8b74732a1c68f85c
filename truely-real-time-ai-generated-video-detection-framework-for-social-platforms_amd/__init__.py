"""truely_amd -- MI355X-native implementation of Truely's per-frame visual hot path
(server/model.py::run of the reference): MTCNN detect -> largest-face crop -> FaceNet
(InceptionResnetV1) embedding -> consecutive-frame cosine drift -> 0..100 score -- and, for the embeddings,
FaceGallery / pairwise / cluster_embeddings: enrolment, distance tables, top-k identification, DBSCAN clustering and score
histograms (threshold calibration: roc_from_counts / threshold_at_far) on the device; FaceTracker associates every face of a
clip's frames into tracks and keeps the drift state machine per person; EmbeddingPool / pool_embeddings pool the embeddings of an
identity, a track or a cluster into one exact template; face_quality measures each face (sharpness, exposure, pose, size) into a
weight in [0, 1] and BestShots keeps the best row of every track; ShotDetector / detect_shots find the hard cuts of a clip from
per-frame colour signatures, and FaceTracker ends its tracks there.

Importable as ``truely_amd`` (see truely_amd.py at the repository root; the directory name
required by the build contract is not a valid Python identifier)."""
from . import weights, synthetic  # noqa: F401  (pure numpy, usable without a GPU)

__all__ = ["weights", "synthetic", "Engine", "MTCNN", "InceptionResnetV1", "FaceGallery", "FaceTracker", "EmbeddingPool", "pool_embeddings", "face_quality", "QualityParams", "BestShots", "frame_signatures", "signature_distance", "ShotParams", "ShotDetector", "detect_shots", "pairwise", "cluster_embeddings", "roc_from_counts", "threshold_at_far", "run", "analyze_video"]


def __getattr__(name):
    # GPU-facing pieces are imported lazily so `import truely_amd` works on a CPU-only box
    if name == "Engine":
        from .engine import Engine
        return Engine
    if name == "MTCNN":
        from .mtcnn import MTCNN
        return MTCNN
    if name == "InceptionResnetV1":
        from .inception_resnet_v1 import InceptionResnetV1
        return InceptionResnetV1
    if name in ("FaceGallery", "pairwise", "cluster_embeddings", "roc_from_counts", "threshold_at_far"):
        from . import gallery
        return getattr(gallery, name)
    if name in ("EmbeddingPool", "pool_embeddings"):
        from . import pool
        return getattr(pool, name)
    if name in ("face_quality", "QualityParams", "BestShots"):
        from . import quality
        return getattr(quality, name)
    if name in ("frame_signatures", "signature_distance", "ShotParams", "ShotDetector", "detect_shots"):
        from . import shots
        return getattr(shots, name)
    if name == "FaceTracker":
        from .tracker import FaceTracker
        return FaceTracker
    if name in ("run", "analyze_video"):
        from . import model
        return getattr(model, name)
    raise AttributeError(name)
