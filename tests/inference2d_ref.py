"""TEST INFRASTRUCTURE, never imported by the product: the reference's test_single_volume (2D/utils.py:63-110), calculate_metric_percase
(:50-60), inference loop (2D/trainer_MaxViT_deform_LKA.py:25-47) and the resize tail of Synapse_dataset.__getitem__
(2D/datasets/dataset_synapse.py:109-126) restated with scipy.ndimage.zoom, torch on the CPU and tests/metrics_ref.py.  The reference's own
files cannot be imported here: they need medpy, SimpleITK and torchvision.  Needs scipy; the GPU tests read only the fixture recorded from it
(tests/golden/reference_inference2d.pt)."""
import numpy as np
import torch

from tests import metrics_ref as MR


def zoom_slices(x, out_hw, order):
    """scipy.ndimage.zoom of every slice with the factors the reference passes: patch / extent."""
    from scipy.ndimage import zoom
    h, w = x.shape[1:]
    return np.stack([zoom(s, (out_hw[0] / h, out_hw[1] / w), order=order) for s in x])


def normalize(x, mean=0.5, std=0.5):
    """ToTensor and Normalize([mean], [std]) of a float32 slice: float32 throughout."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return (t - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)


def calculate_metric_percase(pred, gt):
    pred, gt = np.asarray(pred) > 0, np.asarray(gt) > 0
    if pred.sum() > 0 and gt.sum() > 0:
        return MR.dc(pred, gt), MR.hd95(pred, gt)
    if pred.sum() > 0 and gt.sum() == 0:
        return 1, 0
    return 0, 0


def single_volume(image, label, net, classes, patch_size):
    """(metric_list, prediction, gap): the reference's loop, one slice and one batch-1 forward at a time.  ``gap`` is the difference of the two
    largest logits at the source pixel the order-0 zoom back selects for each output pixel (inf where the zoom gives cval)."""
    from scipy.ndimage import zoom
    image, label = np.asarray(image)[0], np.asarray(label)[0]
    net.eval()
    if image.ndim == 3:
        prediction = np.zeros_like(label)
        gap = np.zeros(label.shape, dtype=np.float64)
        for ind in range(image.shape[0]):
            s = image[ind]
            x, y = s.shape
            resized = x != patch_size[0] or y != patch_size[1]
            if resized:
                s = zoom(s, (patch_size[0] / x, patch_size[1] / y), order=3)
            with torch.no_grad():
                outputs = net(normalize(s)[None, None])
                out = torch.argmax(torch.softmax(outputs, dim=1), dim=1)[0].numpy()
                top = torch.topk(outputs[0].double(), 2, dim=0).values
                g = (top[0] - top[1]).numpy()
            if resized:
                pred = zoom(out, (x / patch_size[0], y / patch_size[1]), order=0)
                # the gap travels with the label: the same order-0 gather (gap + 1 > 0, so cval 0 marks "outside")
                g = zoom(g + 1.0, (x / patch_size[0], y / patch_size[1]), order=0)
                g = np.where(g == 0.0, np.inf, g - 1.0)
            else:
                pred = out
            prediction[ind] = pred
            gap[ind] = g
    else:
        with torch.no_grad():
            outputs = net(torch.from_numpy(image)[None, None].float())
            prediction = torch.argmax(torch.softmax(outputs, dim=1), dim=1)[0].numpy()
            top = torch.topk(outputs[0].double(), 2, dim=0).values
            gap = (top[0] - top[1]).numpy()
    metric_list = [calculate_metric_percase(prediction == i, label == i) for i in range(1, classes)]
    return metric_list, prediction, gap


def inference(net, cases, classes, img_size):
    """(performance, mean_hd95) over ``cases`` = [(image with batch axis, label with batch axis), ...]."""
    total = 0.0
    for image, label in cases:
        total = total + np.array(single_volume(image, label, net, classes, [img_size, img_size])[0], dtype=np.float64)
    total = total / len(cases)
    return float(np.mean(total, axis=0)[0]), float(np.mean(total, axis=0)[1])


def resize_sample(image, label, img_size, mean=0.5, std=0.5):
    """The tail of __getitem__ for every slice of a batch: both arrays zoomed when the slice has another size, ToTensor / Normalize."""
    from scipy.ndimage import zoom
    imgs, labs = [], []
    for im, lb in zip(image, label):
        x, y = im.shape
        if x != img_size or y != img_size:
            im = zoom(im, (img_size / x, img_size / y), order=3)
            lb = zoom(lb, (img_size / x, img_size / y), order=0)
        imgs.append(normalize(im, mean, std)[None])
        labs.append(torch.from_numpy(np.ascontiguousarray(lb))[None])
    return {"image": torch.stack(imgs), "label": torch.stack(labs)}
