from .transform import (BinaryMaskToConnectComponent, Compose, FillHoles3D, RandomAffinePatchCrop3D, RandomBrightness3D,
                        RandomContrast3D, RandomElasticAffinePatchCrop3D, RandomFlip3D, RandomGamma3D, RandomGaussianBlur3D, RandomGaussianNoise3D,
                        RandomLowResolution3D, RandomPatchCrop3D, RandomResizedCrop3D, RandomRotation3D, Resize3D,
                        TopkLargestConnectComponent)
