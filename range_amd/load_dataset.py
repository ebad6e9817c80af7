"""Drop-in for the reference's range/utils/load_dataset.py:9-83, for the one task family that needs no
data file: ``checker_<num_support>`` (range_amd/checker.py).  The other families read CSV files of the
reference's authors and are refused by name."""
from __future__ import annotations

from torch.utils.data import DataLoader

CSV_TASKS = ("biome", "ecoregion", "country", "ocean", "temperature", "housing", "elevation", "population",
             "inat_1", "csv_data")


def get_dataset(args):
    """``args.task_name`` 'checker_<num_support>' -> (train_loader, val_loader, num_classes): 16 classes,
    10 000 samples, train = the seed-0 draw, val = the evaluation lattice; the loaders yield (lonlat, label)
    batches of ``args.batch_size`` in order.  ``args.device`` (optional): the GPU that labels the samples."""
    task = args.task_name
    if task in CSV_TASKS or "era5" in task:
        raise NotImplementedError(f"task {task!r} reads a CSV file of the reference's evaluation data; only the "
                                  "generated 'checker_<num_support>' tasks are built here")
    if "checker" not in task:
        raise ValueError("Task name not recognized")
    from .checker import CheckerDataset
    num_support = int(task.split("_")[-1])
    num_classes = 16
    ds = CheckerDataset(num_samples=10000, num_classes=num_classes, num_support=num_support,
                        device=getattr(args, "device", None))
    kw = dict(batch_size=args.batch_size, num_workers=args.num_workers, shuffle=False, drop_last=False)
    return DataLoader(ds.train_ds, **kw), DataLoader(ds.evalu_ds, **kw), num_classes
