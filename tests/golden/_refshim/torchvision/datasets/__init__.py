"""Names only (see ../__init__.py): nothing here is ever instantiated by the fixture generators."""


class VisionDataset:
    pass


class ImageFolder(VisionDataset):
    pass
