"""MI355X-native Robust U-Net training path (gfx950 HIP kernels behind a C ABI).

The directory name carries the reference repository's name, so import it with
`importlib.import_module("eusipco-2026-robust-unet_amd")`.

Public surface (mirrors /root/reference/Main_Final.py for the hot path):
  RobustUNet, ResidualBlock, DilatedBlock, AttentionGate, ChannelAttention, SpatialAttention
  CoastalDataset, prepare_dataset, ModelEvaluator;  DeepLabV3Plus (baseline);  UNet (train_water_segmentation.py's 2-class model);
  SegNet (comne.py's baseline);  YOLOSeg (Main_Final.py's YOLO-style baseline);  SegFormerLite (Extended_Baseline_Comparison.py's
  transformer baseline);  HRNetWater (the same script's multi-resolution baseline);  WaterNet / WaterIndexModule (its water-index U-Net baseline);
  MSWNet / MultiScaleBlock (its multi-scale baseline);  FastSCNN with DepthwiseSeparableConv, LearningToDownsample, PyramidPoolingFastSCNN,
  GlobalFeatureExtractor, FeatureFusionModule and Classifier (comne.py's depthwise-separable baseline);
  ENet with InitialBlock and BottleneckBlock (comne.py's asymmetric / dilated bottleneck baseline);
  PSPNet with PyramidPooling (comne.py's pyramid-pooling baseline);
  CoastlineExtractor (predict_coastline.py's predictor: device post-processing, native-resolution tiling) and
  trace_external_contours_device (its cv2.findContours step as parallel border following on the device)
  enhance_scene, convert_scene, band_percentiles, select_bands, percentile_ranks (scene.py: the multi-band raster -> uint8 RGB step of
  tif_to_image.py / predict_coastline.py on the device: exact 2-98 % percentiles and the float64 stretch)
  combined_overlay, ndwi_histograms, rgb_histograms, coastline_lengths, analysis_report, create_coastsat_style_visualization,
  error_overlays, generate_error_maps (report.py: the arrays of the reference's analysis report and error-map figures on the device, bit
  for bit numpy's; matplotlib only draws them)
  DeviceCoastalDataset, DeviceLoader, Augment, prepare_device_dataset, resize_pil_device, resample_tables, nearest_table, rotation_words
  (device_data.py: the dataset built once and kept on the device as bytes, PIL-exact resampling there, batches assembled on the device with
  the augmentation of train_water_segmentation.py:313-321)
  distance_transform_sq, distance_transform_sq_host, coastline_deviation, boundary_scores, evaluate_coastline (boundary.py: the exact
  Euclidean distance transform on the device and the coastline-accuracy scores on top of it)
  label_components, label_components_host, dense_labels, water_bodies, clean_water_mask (components.py: connected-component labelling on
  the device, the table of water bodies and the area filter that cleans a water mask in front of the coastline)
plus the MI355X additions: FusedAdam, sigmoid-free fused BCE loss, GradAllReducer (RCCL).

Sub-modules are imported lazily so that host-only pieces (data, portable_rng) stay usable
on a machine without the HIP library; anything that computes raises if
`csrc/librunet_hip.so` is missing — there is no CPU fallback.
"""
import importlib as _il
import os as _os
import sys as _sys

# The backward pass uses several HIP streams (main chain, weight gradients, gradient all-reduce + RCCL's own): with HIP's default of 4 hardware
# queues they share queues and serialise on each other's event waits (380 vs 414 img/s).  The variable only counts if it is set before the HIP
# runtime comes up, so it is set here, when the package is imported - normally long before the first device call.
_HW_QUEUES_LATE = False
if "GPU_MAX_HW_QUEUES" not in _os.environ:
    _os.environ["GPU_MAX_HW_QUEUES"] = "8"
    _t = _sys.modules.get("torch")
    _HW_QUEUES_LATE = bool(_t is not None and _t.cuda.is_available() and _t.cuda.is_initialized())

_LAZY = {
    "RobustUNet": "model", "ResidualBlock": "model", "DilatedBlock": "model", "AttentionGate": "model",
    "ChannelAttention": "model", "SpatialAttention": "model", "DeepLabV3Plus": "deeplab", "ASPP": "deeplab",
    "CoastalDataset": "data", "prepare_dataset": "data", "synthetic_batch": "data", "DevicePrefetcher": "data",
    "ModelEvaluator": "evaluator", "FusedAdam": "optim", "bce_loss": "ops", "GradAllReducer": "ddp",
    "TrainStep": "trainer", "fit": "trainer", "UNet": "unet", "cross_entropy": "ops", "bilinear_resize": "ops",
    "SegNet": "segnet", "YOLOSeg": "yolo", "SegFormerLite": "segformer", "CoastlineExtractor": "predict",
    "HRNetWater": "hrnet", "WaterNet": "waternet", "WaterIndexModule": "waternet", "MSWNet": "mswnet", "MultiScaleBlock": "mswnet",
    "FastSCNN": "fastscnn", "DepthwiseSeparableConv": "fastscnn", "LearningToDownsample": "fastscnn", "PyramidPoolingFastSCNN": "fastscnn",
    "GlobalFeatureExtractor": "fastscnn", "FeatureFusionModule": "fastscnn", "Classifier": "fastscnn",
    "ENet": "enet", "InitialBlock": "enet", "BottleneckBlock": "enet",
    "PSPNet": "pspnet", "PyramidPooling": "pspnet",
    "enhance_scene": "scene", "convert_scene": "scene", "band_percentiles": "scene", "select_bands": "scene", "percentile_ranks": "scene",
    "trace_external_contours_device": "predict",
    "combined_overlay": "report", "ndwi_histograms": "report", "rgb_histograms": "report", "coastline_lengths": "report",
    "analysis_report": "report", "create_coastsat_style_visualization": "report", "error_overlays": "report", "generate_error_maps": "report",
    "DeviceCoastalDataset": "device_data", "DeviceLoader": "device_data", "Augment": "device_data", "prepare_device_dataset": "device_data",
    "resize_pil_device": "device_data", "resample_tables": "device_data", "nearest_table": "device_data", "rotation_words": "device_data",
    "distance_transform_sq": "boundary", "distance_transform_sq_host": "boundary", "coastline_deviation": "boundary",
    "boundary_scores": "boundary", "evaluate_coastline": "boundary",
    "label_components": "components", "label_components_host": "components", "dense_labels": "components", "water_bodies": "components",
    "clean_water_mask": "components",
}


def __getattr__(name):
    if name in _LAZY:
        return getattr(_il.import_module(f"{__name__}.{_LAZY[name]}"), name)
    raise AttributeError(name)


__all__ = sorted(_LAZY)
