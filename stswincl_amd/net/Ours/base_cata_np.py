"""Drop-in for ``net.Ours.base_cata_np`` of the CaDIS package (segcata/net/Ours/base_cata_np.py:49-108): ``TswinPlusv5`` is
TswinPlus with the CaDIS input resolution (64, 80) of the Swin feature map, i.e. 512 x 640 input frames.  Not to be confused with
``contrast.models.Ours.base.TswinPlusv5``, whose default is (32, 56)."""
from .base18 import TswinPlus


class TswinPlusv5(TswinPlus):
    def __init__(self, num_classes, input_resolution=(64, 80)):
        super().__init__(num_classes, input_resolution)
