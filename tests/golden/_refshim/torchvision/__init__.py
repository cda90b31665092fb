"""Stand-in for the uninstalled `torchvision`: the reference's train_utils/datasets.py imports
`torchvision.datasets.ImageFolder` / `VisionDataset` at module top, and tests/golden/make_golden_vae_encode.py only
needs that module's `center_crop_arr`.  Used only by the fixture generators."""
