"""Host restatement of CPD's box tracker (cpd/unsupervised_core/tracker/tracker.py Tracker3D, trajectory.py Trajectory, object.py
Object, box_op.py register_bbs / convert_bbs_type) and of outline_utils.py TrackSmooth (l.968-1120), which MFCF (and OYSTER)
run over a sequence's per-frame boxes. A sequential 13-state constant-acceleration Kalman filter over a few hundred boxes per
frame: it stays numpy on the host; plain arrays stand in for the reference's np.mat, the products and their
order are the reference's.

State: x y z, vx vy vz, ax ay az, l w h yaw. Config keys (attribute or dict, read through outline._get): state_func_covariance,
measure_func_covariance, prediction_score_decay, LiDAR_scanning_frequency, max_prediction_num,
max_prediction_num_for_new_object, lwh_win_size, yaw_win_size, init_score, update_score, latency, remove_short_track, and the
class tables of outline.get_box_cls."""
import numpy as np

from .outline import _get, get_box_cls

STATE_DIM, BOX_DIM = 13, 7


def convert_bbs_type(boxes, input_box_type):
    """box_op.py:4-25 for the (x, y, z, l, w, h, yaw) box types: a copy of the boxes. The 'Kitti' reordering, which nothing in
    the pseudo-label generators asks for, is not restated."""
    assert input_box_type in ["Kitti", "OpenPCDet", "Waymo"], 'unsupported input box type!'
    if input_box_type == "Kitti":
        raise NotImplementedError("cpd_amd.tracker: box type 'Kitti' is not restated (TrackSmooth tracks 'OpenPCDet' boxes)")
    return np.array(boxes)


def get_registration_angle(mat):
    cos_theta, sin_theta = mat[0, 0], mat[1, 0]
    cos_theta = min(max(cos_theta, -1), 1)
    theta_cos = np.arccos(cos_theta)
    return theta_cos if sin_theta >= 0 else 2 * np.pi - theta_cos


def register_bbs(boxes, pose):
    """box_op.py:44-63: the centres through `pose`, the headings turned by its angle. `boxes` is rewritten IN PLACE and
    returned, as in the reference."""
    if pose is None:
        return boxes
    pose = np.asarray(pose)
    ang = get_registration_angle(pose)
    ones = np.ones(shape=(boxes.shape[0], 1))
    for b in range(0, boxes.shape[1] // 7 * 7, 7):
        box_world = np.matmul(np.concatenate([boxes[:, b:b + 3], ones], -1), pose.T)
        boxes[:, b:b + 3] = box_world[:, 0:3]
        boxes[:, b + 6] += ang
    return boxes


def points_rigid_transform(cloud, pose):
    """trajectory.py:263-272: float32 rows through the float64 product, rounded to float32."""
    if cloud.shape[0] == 0:
        return cloud
    mat = np.ones(shape=(cloud.shape[0], 4), dtype=np.float32)
    mat[:, 0:3] = cloud[:, 0:3]
    return np.array((np.asarray(pose) @ mat.astype(np.float64).T).T, dtype=np.float32)[:, 0:3]


class Object:
    """object.py: one timestamp of a trajectory; states are [13, 1] columns, the detection a [7, 1] column."""

    def __init__(self):
        self.updated_state = None
        self.predicted_state = None
        self.detected_state = None
        self.updated_covariance = None
        self.predicted_covariance = None
        self.prediction_score = None
        self.score = None
        self.features = None


def _limit(ang):
    ang = ang % (2 * np.pi)
    ang[ang > np.pi] = ang[ang > np.pi] - 2 * np.pi
    ang[ang < -np.pi] = ang[ang < -np.pi] + 2 * np.pi
    return ang


def _softmax(x):
    x = x - x.max(axis=-1).reshape(list(x.shape)[:-1] + [1])
    e = np.exp(x)
    return e / e.sum(axis=-1).reshape(list(x.shape)[:-1] + [1])


def _sigmoid(x):
    return 1.0 / (1 + np.exp(-float(x)))


class Trajectory:
    """trajectory.py Trajectory for boxes without features (tracking_features False, as TrackSmooth builds its tracker)."""

    def __init__(self, init_bb=None, init_features=None, init_score=None, init_timestamp=None, label=None,
                 tracking_features=False, bb_as_features=False, config=None):
        assert init_bb is not None
        if tracking_features or bb_as_features:
            raise NotImplementedError("cpd_amd.tracker: feature tracking is not restated (TrackSmooth never asks for it)")
        self.init_bb, self.init_score, self.init_timestamp, self.label, self.config = init_bb, init_score, init_timestamp, label, config
        self.scanning_interval = 1. / _get(config, "LiDAR_scanning_frequency")
        self.trajectory = {}
        self.track_dim = STATE_DIM
        self.init_parameters()
        self.init_trajectory()
        self.consecutive_missed_num = 0
        self.first_updated_timestamp = init_timestamp
        self.last_updated_timestamp = init_timestamp

    def __len__(self):
        return len(self.trajectory)

    def init_parameters(self):
        """l.114-137. B picks (x y z, l w h yaw) out of the state; it is taken from A before A gets its motion terms."""
        n, dt = STATE_DIM, self.scanning_interval
        self.A = np.eye(n)
        self.Q = np.eye(n) * _get(self.config, "state_func_covariance")
        self.P = np.eye(BOX_DIM) * _get(self.config, "measure_func_covariance")
        self.B = np.zeros((BOX_DIM, n))
        self.B[0:3, :] = self.A[0:3, :]
        self.B[3:, :] = self.A[9:, :]
        self.A[0:3, 3:6] = np.eye(3) * dt
        self.A[3:6, 6:9] = np.eye(3) * dt
        self.A[0:3, 6:9] = np.eye(3) * 0.5 * dt ** 2
        self.H = self.B.T.copy()
        self.K = np.zeros((n, n))
        self.K[3, 0] = self.K[4, 1] = self.K[5, 2] = dt

    def _detected(self, bb):
        return np.asarray(bb, np.float64)[:BOX_DIM].reshape(BOX_DIM, 1).copy()

    def init_trajectory(self):
        """l.74-112: updated and predicted state of the first object are ONE array, as in the reference."""
        detected = self._detected(self.init_bb)
        state = self.H @ detected
        cov = (np.eye(STATE_DIM) * 0.01).T
        ob = Object()
        ob.updated_state = ob.predicted_state = state
        ob.detected_state = detected
        ob.updated_covariance = ob.predicted_covariance = cov
        ob.prediction_score = 1
        ob.score = self.init_score
        self.trajectory[self.init_timestamp] = ob

    def state_prediction(self, timestamp):
        """l.139-178."""
        assert timestamp - 1 in self.trajectory
        prev = self.trajectory[timestamp - 1]
        decay = _get(self.config, "prediction_score_decay")
        if prev.updated_state is not None:
            state, cov = prev.updated_state, prev.updated_covariance
            score = prev.prediction_score * (1 - decay * 15)
        else:
            state, cov = prev.predicted_state, prev.predicted_covariance
            score = prev.prediction_score * (1 - decay)
        ob = Object()
        ob.predicted_state = self.A @ state
        ob.predicted_covariance = self.A @ cov @ self.A.T + self.Q
        ob.prediction_score = score
        self.trajectory[timestamp] = ob
        self.consecutive_missed_num += 1

    def state_update(self, bb=None, features=None, score=None, timestamp=None):
        """l.183-252; the second object of a trajectory takes its velocity from the two detections (len == 2)."""
        assert bb is not None
        assert timestamp in self.trajectory
        detected = self._detected(bb)
        ob = self.trajectory[timestamp]
        pred, pcov = ob.predicted_state, ob.predicted_covariance
        temp = self.B @ pcov @ self.B.T + self.P
        gain = pcov @ self.B.T @ np.linalg.inv(temp)
        updated = pred + gain @ (detected - self.B @ pred)
        ucov = (np.eye(STATE_DIM) - gain @ self.B) @ pcov
        if len(self.trajectory) == 2:
            updated = self.H @ detected + self.K @ (self.H @ detected - self.trajectory[timestamp - 1].updated_state)
        ob.updated_state, ob.updated_covariance, ob.detected_state = updated, ucov, detected
        decay = _get(self.config, "prediction_score_decay")
        if self.consecutive_missed_num > 1:
            ob.prediction_score = 1
        elif self.trajectory[timestamp - 1].updated_state is not None:
            ob.prediction_score = ob.prediction_score + decay * 15 * _sigmoid(score)
        else:
            ob.prediction_score = ob.prediction_score + decay * _sigmoid(score)
        ob.score = score
        ob.features = features
        self.consecutive_missed_num = 0
        self.last_updated_timestamp = timestamp

    def filtering(self, config, pose=None):
        """l.384-520: the global smoothing pass of latency < 0, which every shipped config sets. The near-online branch of
        latency >= 0 (l.521-542) is not restated."""
        wind_size = int(_get(config, "LiDAR_scanning_frequency") * _get(config, "latency"))
        if wind_size >= 0:
            raise NotImplementedError("cpd_amd.tracker: latency >= 0 (near-online filtering) is not restated; the shipped "
                                      "configs set latency: -1")
        max_pred = _get(config, "max_prediction_num")
        all_scores, size, dist = [], {}, {}
        for key, ob in self.trajectory.items():
            if ob.score is not None:
                all_scores.append(ob.score)
            if self.first_updated_timestamp <= key <= self.last_updated_timestamp and ob.updated_state is None:
                # a missed frame inside the track: between the nearest states on either side, each weighted by its OWN distance
                left, n_left, k = None, 0, key - 1
                while left is None and k > key - max_pred:
                    left, n_left, k = self.trajectory[k].updated_state, n_left + 1, k - 1
                right, n_right, k = None, 0, key + 1
                while right is None and k < key + max_pred:
                    right, n_right, k = self.trajectory[k].updated_state, n_right + 1, k + 1
                if left is not None and right is not None:
                    sums = n_left + n_right
                    for d in range(3):
                        ob.predicted_state[d, 0] = (n_left / sums) * left[d, 0] + (n_right / sums) * right[d, 0]
                ob.updated_state = ob.predicted_state
            if ob.updated_state is not None:
                s = ob.updated_state
                if s[9, 0] < s[10, 0]:
                    s[9, 0], s[10, 0] = s[10, 0], s[9, 0]
                    s[12, 0] += np.pi / 2
                here = points_rigid_transform(np.array([[s[0, 0], s[1, 0], s[2, 0]]]), np.linalg.inv(pose[key]))
                dist[key] = np.linalg.norm(here)
                size[key] = (s[9, 0], s[10, 0], s[11, 0], s[12, 0])
        lwh_win, yaw_win = _get(config, "lwh_win_size"), _get(config, "yaw_win_size")
        mean_score = np.mean(all_scores)
        for key, ob in self.trajectory.items():
            if ob.updated_state is not None and lwh_win > 0:
                near = [k for k in range(key - lwh_win, key + lwh_win) if k in size]
                yaws = [size[k][3] for k in range(key - yaw_win, key + yaw_win) if k in size]
                d = np.array([[dist[k] for k in near]])
                d -= d.min()
                d /= d.max() + 0.1
                d = 1 - d + 0.1
                weights = _softmax(d)[0]
                new_ya = ob.updated_state[12, 0]
                res = _limit(_limit(np.array(yaws)) - new_ya)
                res = res[np.abs(res) < 2]
                ob.updated_state[12, 0] = new_ya + res.mean()
                for j in range(3):
                    ob.updated_state[9 + j, 0] = np.sum(np.array([size[k][j] for k in near]) * weights)
            ob.score = mean_score


class Tracker3D:
    """tracker.py Tracker3D."""

    def __init__(self, tracking_features=False, bb_as_features=False, box_type='Kitti', config=None):
        self.config = config
        self.current_timestamp = self.current_pose = self.current_bbs = self.current_features = self.current_scores = None
        self.tracking_features, self.bb_as_features, self.box_type = tracking_features, bb_as_features, box_type
        self.label_seed = 0
        self.active_trajectories = {}
        self.dead_trajectories = {}

    def _new(self, box, score, label):
        return Trajectory(init_bb=box, init_score=score, init_timestamp=self.current_timestamp, label=label,
                          tracking_features=self.tracking_features, bb_as_features=self.bb_as_features, config=self.config)

    def tracking(self, bbs_3D=None, features=None, scores=None, pose=None, timestamp=None):
        """l.32-71: (tracked boxes in world coordinates, their ids). An empty frame arrives as []."""
        self.current_bbs, self.current_features, self.current_scores = bbs_3D, features, scores
        self.current_pose, self.current_timestamp = pose, timestamp
        self.trajectores_prediction()
        if self.current_bbs is None or len(self.current_bbs) == 0:
            return np.zeros(shape=(0, 7)), np.zeros(shape=(0))
        self.current_bbs = convert_bbs_type(self.current_bbs, self.box_type)
        self.current_bbs = register_bbs(self.current_bbs, self.current_pose)
        ids = self.association()
        bbs, ids = self.trajectories_update_init(ids)
        return np.array(bbs), np.array(ids)

    def trajectores_prediction(self):
        """l.75-98: a track dies after max_prediction_num misses (and is not predicted again), a one-hit track once it is
        max_prediction_num_for_new_object long (after one more prediction)."""
        dead = []
        for key, tra in self.active_trajectories.items():
            if tra.consecutive_missed_num >= _get(self.config, "max_prediction_num"):
                dead.append(key)
                continue
            if len(tra) - tra.consecutive_missed_num == 1 and len(tra) >= _get(self.config, "max_prediction_num_for_new_object"):
                dead.append(key)
            tra.state_prediction(self.current_timestamp)
        for key in dead:
            self.dead_trajectories[key] = self.active_trajectories.pop(key)

    def compute_cost_map(self):
        """l.100-168: [detections, active trajectories]. The angle term reads state 11 (the height), as the reference does."""
        all_ids = list(self.active_trajectories.keys())
        pred = np.array([np.concatenate([np.array(t.trajectory[self.current_timestamp].predicted_state).reshape(-1),
                                         np.array([t.trajectory[self.current_timestamp].prediction_score])])
                         for t in self.active_trajectories.values()])
        det = np.array([self._new(box, self.current_scores[i], 1).trajectory[self.current_timestamp].predicted_state.reshape(-1)
                        for i, box in enumerate(self.current_bbs)])
        det, pred = det[:, None, :], pred[None, :, :]
        dis = np.sqrt(((det[..., 0:3] - pred[..., 0:3]) ** 2).sum(-1))
        whl_dis = (np.abs(det[..., 9:11] - pred[..., 9:11]) / (det[..., 9:11] + pred[..., 9:11] + 0.00001)).sum(-1)
        angle_dis = 1 - np.cos(det[..., 11] - pred[..., 11])
        return (dis + 0.1 * whl_dis + 1 * angle_dis) * pred[..., -1], all_ids

    def association(self):
        """l.170-195: greedy in detection order; a taken trajectory's column is blanked with 100000."""
        n = len(self.current_bbs)
        if len(self.active_trajectories) == 0:
            ids = list(range(self.label_seed, self.label_seed + n))
            self.label_seed += n
            return ids
        ids = []
        cost_map, all_ids = self.compute_cost_map()
        for i in range(n):
            arg_min = np.argmin(cost_map[i])
            if cost_map[i][arg_min] < 3.:
                ids.append(all_ids[arg_min])
                cost_map[:, arg_min] = 100000
            else:
                ids.append(self.label_seed)
                self.label_seed += 1
        return ids

    def trajectories_update_init(self, ids):
        """l.198-243."""
        assert len(ids) == len(self.current_bbs)
        valid_bbs, valid_ids = [], []
        for i, label in enumerate(ids):
            box, score = self.current_bbs[i], self.current_scores[i]
            features = None if self.current_features is None else self.current_features[i]
            if label in self.active_trajectories and score > _get(self.config, "update_score"):
                self.active_trajectories[label].state_update(bb=box, features=features, score=score,
                                                             timestamp=self.current_timestamp)
            elif score > _get(self.config, "init_score"):
                self.active_trajectories[label] = self._new(box, score, label)
            else:
                continue
            valid_bbs.append(box)
            valid_ids.append(label)
        if len(valid_bbs) == 0:
            return np.zeros(shape=(0, 7)), np.zeros(shape=(0))
        return np.array(valid_bbs), np.array(valid_ids)

    def post_processing(self, config, pose=None):
        """l.246-265: every trajectory filtered; the dead ones first, then the active ones."""
        tra = {}
        for group in (self.dead_trajectories, self.active_trajectories):
            for key, track in group.items():
                track.filtering(config, pose=pose)
                tra[key] = track
        return tra


class TrackSmooth:
    """outline_utils.py:968-1120 (tracking, get_current_frame_objects_and_cls)."""

    def __init__(self, config):
        self.tracker_config = config
        self.tracker = Tracker3D(box_type='OpenPCDet', config=self.tracker_config)

    def tracking(self, all_objects, all_pose, scores=None):
        self.all_pose = all_pose
        for i, boxes in enumerate(all_objects):
            s = np.ones(shape=(len(boxes),)) * 100 if scores is None else scores[i]
            self.tracker.tracking(boxes, scores=s, timestamp=i, pose=all_pose[i])
        tracks = self.tracker.post_processing(self.tracker_config, self.all_pose)
        self.frame_first_dict = {}
        for ob_id, track in tracks.items():
            if track.last_updated_timestamp - track.first_updated_timestamp < _get(self.tracker_config, "remove_short_track"):
                continue
            states = {f: np.array(ob.updated_state.T) for f, ob in track.trajectory.items() if ob.updated_state is not None}
            all_position = np.array([s[0, 0:3] for s in states.values()])
            all_speed = np.array([s[0, 3:6] for s in states.values()])
            std = np.std(np.linalg.norm(all_position[:, 0:2] - np.mean(all_position[:, 0:2], 0), axis=1))
            speed = np.mean(np.linalg.norm(all_speed, axis=1))
            for frame_id, s in states.items():
                self.frame_first_dict.setdefault(frame_id, []).append((ob_id, s, std, speed, track.trajectory[frame_id].score))

    def get_current_frame_objects_and_cls(self, frame_id, return_name=True):
        """l.1030-1120: the frame's tracked boxes back in its own coordinates, ids, class names (or numbers) and dif. The class
        chain reads the box after it is registered (its z is the frame's), as the reference does."""
        empty = (np.empty(shape=(0, 7)), np.empty(shape=(0,)), np.empty(shape=(0,)), np.empty(shape=(0,)))
        if frame_id not in self.frame_first_dict or len(self.frame_first_dict[frame_id]) == 0:
            return empty
        new_pose = np.linalg.inv(self.all_pose[frame_id])
        objects, obj_ids = [], []
        for ob_id, ob_state, _, _, _ in self.frame_first_dict[frame_id]:
            box = np.zeros(shape=(1, 7))
            box[0, 0:3] = ob_state[0, 0:3]
            box[0, 3:7] = ob_state[0, 9:13]
            objects.append(register_bbs(box, new_pose))
            obj_ids.append(ob_id)
        objects = np.concatenate(objects)
        _, cls, dif = get_box_cls(objects, self.tracker_config)
        if not return_name:
            proto = _get(self.tracker_config, "cls")
            cls = np.array([proto[c] for c in cls])
        return objects, np.array(obj_ids), cls, dif
