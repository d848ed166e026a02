"""Vision front end (reference: src/kompass_core/vision.py): `DepthDetector` turns 2-D detections on an aligned
uint16 depth frame into 3-D boxes; the per-pixel work runs on the MI355X in one launch per frame."""
from kompass_cpp.vision import DepthDetector

__all__ = ["DepthDetector"]
