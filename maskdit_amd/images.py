"""Image-side input of latent extraction (extract_latent.py): the ImageFolder enumeration and the ADM center crop that
the reference's `imagenet_lmdb_dataset` applies (train_utils/datasets.py:19-37, 55-124), with PIL + numpy only -- no
torchvision.  Host code; the pixels go to the GPU as uint8 NHWC batches (FrozenAutoencoderKL.encode_moments)."""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np

# torchvision.datasets.folder.IMG_EXTENSIONS (what ImageFolder accepts), compared case-insensitively
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')


def image_folder_samples(root: str) -> Tuple[List[Tuple[str, int]], List[str]]:
    """`ImageFolder(root).samples` / `.classes`: classes = the sorted sub-directory names (label = index), samples in
    class-major order, each class's files by `sorted(os.walk(...))` directory then sorted file name."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f'{root}: no class directories (expected <root>/<class>/<image>)')
    samples = []
    for label, cls in enumerate(classes):
        for d, _, fnames in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            for f in sorted(fnames):
                if f.lower().endswith(IMG_EXTENSIONS):
                    samples.append((os.path.join(d, f), label))
    return samples, classes


def center_crop_arr(pil_image, image_size: int) -> np.ndarray:
    """ADM center crop (train_utils/datasets.py:19-37): halve with BOX while the short side is >= 2 x the target, scale
    the short side to the target with BICUBIC, crop the center.  Returns the uint8 array (the reference wraps it in
    Image.fromarray, which ToTensor turns back into the same bytes)."""
    from PIL import Image
    while min(*pil_image.size) >= 2 * image_size:
        pil_image = pil_image.resize(tuple(x // 2 for x in pil_image.size), resample=Image.BOX)
    scale = image_size / min(*pil_image.size)
    pil_image = pil_image.resize(tuple(round(x * scale) for x in pil_image.size), resample=Image.BICUBIC)
    arr = np.array(pil_image)
    crop_y = (arr.shape[0] - image_size) // 2
    crop_x = (arr.shape[1] - image_size) // 2
    return arr[crop_y: crop_y + image_size, crop_x: crop_x + image_size]


def load_rgb_crop(path: str, image_size: int) -> np.ndarray:
    """One dataset item as ImageLMDB.__getitem__ decodes it (datasets.py:109-119): RGB, center crop -> uint8 [R, R, 3]."""
    from PIL import Image
    with Image.open(path) as im:
        return center_crop_arr(im.convert('RGB'), image_size)
