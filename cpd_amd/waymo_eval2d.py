"""BEV-protocol Waymo detection metrics (L1 / L2 AP and APH per object type) on the GPU: a drop-in for
cpd/datasets/waymo_unsupervised/waymo_eval2d.py with no tensorflow / waymo_open_dataset dependency. This is the protocol
unsupervised-detection tables (OYSTER and after) are reported under: box_type TYPE_2D, IoU 0.5 / 0.3 / 0.3 / 0.3.

Same public surface as the reference file: OpenPCDetWaymoDetectionMetricsEstimator (a plain class here) with
WAYMO_CLASSES, generate_waymo_type_results, mask_by_distance, build_config and waymo_evaluation(prediction_infos, gt_infos,
class_name, distance_thresh=100, fake_gt_infos=True) -> {'OBJECT_TYPE_TYPE_<T>_LEVEL_<L>/AP' | '/APH': [float]} in the
order VEHICLE, PEDESTRIAN, SIGN, CYCLIST x LEVEL_1, LEVEL_2 x AP, APH; module-level limit_period and main(). Added:
waymo_evaluation_at(..., iou_thresholds) for several threshold sets over one pass of IoU blocks.

PARITY STATUS. As for cpd_amd.waymo_eval: the metric itself is implemented inside waymo_open_dataset, not in the reference
tree; it was neither run nor read. What is computed here is the published definition -- the reference's metric config
(waymo_eval2d.py:87-109) and the AP / APH formulas of the Waymo Open Dataset paper (Sun et al., CVPR 2020, section 5.1) --
restated as the protocol below. No bit-parity with the official tool is claimed. Known unknowns, the same four:
  * Recall interpolation. The official AP routine takes a max_recall_delta and is believed to insert interpolated points
    where neighbouring operating points lie more than 0.05 apart in recall. That is not reproduced; values can differ
    from the official tool's where the PR curve has such gaps.
  * Tie handling. The official Hungarian matcher may quantise IoU to integers before matching. Here the weights are
    float64; when two matchings of a problem tie, or nearly tie, in total IoU, the choice may differ.
  * IoU near a threshold. The official IoU comes from its own polygon code; pairs within rounding of a threshold can
    fall on the other side.
  * APL. Later library versions also emit '/APL'. It is not produced here.

PROTOCOL. cpd_amd.waymo_eval's (cut-offs, matching, levels, counts, heading accuracy, AP / APH: see its docstring), with
two differences. Type ids 1..4 have IoU thresholds 0.5, 0.3, 0.3, 0.3. Boxes are float32 rows (cx, cy, dx, dy, heading) --
columns [0, 1, 3, 4, 6] of the seven-column boxes, taken after the fake-lidar conversion (waymo_eval2d.py:61-63, 68-69) --
and IoU = area of the intersection of the two rotated rectangles / (dx_a dy_a + dx_b dy_b - that area), float64: height
plays no part, so a prediction above or below a ground truth with the same footprint matches it. IoU is 0 for an empty
intersection, a non-positive union, a size that is not positive, a non-finite value, and any value of magnitude 2^29 or
more (which holds neither a position nor a direction in float32).

WHERE THE WORK RUNS. As in cpd_amd.waymo_eval: masks, conversion and AP integration on the host; per chunk of frames one
cpd_waymo_iou_bev launch and one cpd_waymo_match launch per threshold set; totals stay on the device and are read back
once. Same limits, same CpdHipError without a GPU: there is no CPU fallback.

Differences from the reference's host code, the same two and as deliberate: generate_waymo_type_results does not modify
the caller's infos, and a prediction set with no boxes at all evaluates to zeros where the reference's pd_score.max()
raises.
"""
import argparse
import pickle

from . import waymo_eval
from .waymo_eval import average_precision, limit_period, result_dict  # noqa: F401  (the module's surface)

BOX_TYPE = 'TYPE_2D'
IOU_THRESHOLDS = waymo_eval.BOX_TYPES[BOX_TYPE][3]          # type ids 1..4 (build_config's iou_thresholds[1:])


class OpenPCDetWaymoDetectionMetricsEstimator(waymo_eval.OpenPCDetWaymoDetectionMetricsEstimator):
    """generate_waymo_type_results returns five-column boxes (waymo_eval2d.py:26-85: the same class mask, difficulty rule,
    fake-lidar conversion and heading wrap, then columns [0, 1, 3, 4, 6]); build_config is waymo_eval2d.py:87-109 as a
    plain dict; mask_by_distance, waymo_evaluation (l.179-217) and waymo_evaluation_at are the 3-D estimator's, which
    reads the box type and the columns from here."""
    WAYMO_CLASSES = ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']
    BOX_TYPE = BOX_TYPE
    BOX_COLUMNS = [0, 1, 3, 4, 6]


def main():
    parser = argparse.ArgumentParser(description='arg parser')
    parser.add_argument('--pred_infos', type=str, required=True, help='pickle file')
    parser.add_argument('--gt_infos', type=str, required=True, help='pickle file')
    parser.add_argument('--class_names', type=str, nargs='+', default=['Vehicle', 'Pedestrian', 'Cyclist'], help='')
    parser.add_argument('--sampled_interval', type=int, default=10, help='sampled interval for GT sequences')
    args = parser.parse_args()

    with open(args.pred_infos, 'rb') as f:
        pred_infos = pickle.load(f)
    with open(args.gt_infos, 'rb') as f:
        gt_infos = pickle.load(f)

    print('Start to evaluate the waymo format results...')
    estimator = OpenPCDetWaymoDetectionMetricsEstimator()

    gt_infos_dst = []
    for idx in range(0, len(gt_infos), args.sampled_interval):
        cur_info = gt_infos[idx]['annos']
        cur_info['frame_id'] = gt_infos[idx]['frame_id']
        gt_infos_dst.append(cur_info)

    ap_dict = estimator.waymo_evaluation(
        pred_infos, gt_infos_dst, class_name=args.class_names, distance_thresh=1000, fake_gt_infos=False
    )

    ap_result_str = '\n'
    for key in ap_dict:
        ap_dict[key] = ap_dict[key][0]
        ap_result_str += '%s: %.4f \n' % (key, ap_dict[key])
    print(ap_result_str)


if __name__ == '__main__':
    main()
