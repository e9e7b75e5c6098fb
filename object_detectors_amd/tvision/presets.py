"""Mirror of the reference's detection presets (torchvision_models/detection/presets.py:5-38) for the uint8 route of
`GeneralizedRCNNTransform.ingest`.

    preset = DetectionPresetTrain("hflip", hflip_prob=0.5)
    flips = preset.draw(len(images))                               # one flag per image
    image_list, targets = model.transform.ingest(images, targets, flips)

The reference applies its presets per sample on the host: `RandomHorizontalFlip` (detection/transforms.py:30-44) mirrors the PIL image, the
boxes and the masks, `ToTensor` divides by 255.  Here a preset only DECIDES: the flip itself, the division and everything after it run inside
the ingest kernels.  `draw` consumes torch's global CPU generator exactly as the reference's per-sample `torch.rand(1) < p` does, one draw
per image and in order, so the same seed flips the same images."""
import torch


class DetectionPresetTrain:
    def __init__(self, data_augmentation="hflip", hflip_prob=0.5):
        if data_augmentation in ("ssd", "ssdlite"):
            raise NotImplementedError(f'data augmentation policy "{data_augmentation}": the SSD augmentations need the shapes and the targets, '
                                      "which a preset's draw(n) does not see: use transforms.SSDAugmentation(policy).draw(shapes, targets) "
                                      "and ingest(images, targets, augment=params)")
        if data_augmentation != "hflip":
            raise ValueError(f'Unknown data augmentation policy "{data_augmentation}"')
        self.hflip_prob = hflip_prob

    def draw(self, n):
        """The flip flags of n images: `torch.rand(1) < p` once per image, in order (transforms.py:33)."""
        return [bool(torch.rand(1) < self.hflip_prob) for _ in range(n)]


class DetectionPresetEval:
    def draw(self, n):
        """No augmentation in evaluation: nothing is flipped and no random number is drawn."""
        return [False] * n
