"""range_amd - MI355X-native engine for the RANGE / RANGE+ retrieval-augmented geo-embedding
forward path of mvrl/RANGE (``load_model(...)(locs)``), its batch driver (``save_embeddings``) and
the downstream ridge probe (``evaluate_npz``), with the dataset factory (``get_dataset``) for the generated
checkerboard tasks (``CheckerDataset``) in front, and the embedding map (``embedding_map`` / ``ica_colors`` /
``coord_grid``: the FastICA colours of a model's embeddings) and the cluster map (``cluster_map`` /
``cluster_labels``: their complete-linkage clusters).  See DESIGN.md."""
from .load_model import load_model  # noqa: F401
from .range import LocationEncoder  # noqa: F401
# The embedding map's driver shares its name with its module, so the name is bound here, once, to the function
# (``from range_amd.embedding_map import ...`` still reaches the module); the module itself is light, its binding
# is loaded on first use like the others.
from .embedding_map import coord_grid, embedding_map, ica_colors  # noqa: F401
# ... and so does the cluster map's (complete-linkage clusters of a model's embeddings)
from .cluster_map import cluster_labels, cluster_map  # noqa: F401


def __getattr__(name):
    # the driver and the probe are imported on first use (they pull in their own bindings)
    if name == "save_embeddings":
        from .save import save_embeddings
        return save_embeddings
    if name == "evaluate_npz":
        from .evaluate import evaluate_npz
        return evaluate_npz
    if name == "get_dataset":
        from .load_dataset import get_dataset
        return get_dataset
    if name == "CheckerDataset":
        from .checker import CheckerDataset
        return CheckerDataset
    raise AttributeError(f"module 'range_amd' has no attribute {name!r}")


__all__ = ["load_model", "LocationEncoder", "save_embeddings", "evaluate_npz", "get_dataset", "CheckerDataset",
           "ica_colors", "embedding_map", "coord_grid", "cluster_labels", "cluster_map"]
