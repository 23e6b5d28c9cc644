"""TEST INFRASTRUCTURE ONLY -- pure-Python restatement of the fake detector's tracking histories
and sensor-range getters (the oracle for include/impc_detect.h).  Only tests/ may import it.

Follows onboard_detector/include/onboard_detector/fakeDetector.cpp statement by statement:
  histCB                    :337-347  obstacleHist_ sized on the first call (:338-340); per obstacle
                                      pop_back once histSize_ entries are held (:342-344), then
                                      push_front(obstacleMsg_[i]) (:345)
  isObstacleInSensorRange   :482-500  diff = pObstacle - pRobot (:486), diff(2) = 0 (:487), distance =
                                      diff.norm() (:488), direction = (cos yaw, sin yaw, 0) (:490),
                                      angle = angleBetweenVectors(direction, diff) (:492; utils.h:58-60:
                                      atan2(a.cross(b).norm(), a.dot(b))), true when angle <= fov / 2
                                      and distance <= colorDistance_ (:493)
  getObstaclesInSensorRange :513-523  the boxes of obstacleMsg_ that pass, widths += robotSize
  getDynamicObstaclesHist   :525-556  the histories whose entry [0] passes with fov = 2 pi (:533):
                                      pos, vel = (Vx, Vy, 0) (:537), size + robotSize (:540)
A box is a dict(x, y, z, Vx, Vy, x_width, y_width, z_width) (onboardDetector::box3D; the
acceleration history is not carried: nothing downstream of the getters reads accHist).  Eigen's
norm of a 3-vector is sqrt(x x + y y + z z) summed in that order, its cross product (a1 b2 - a2 b1,
a2 b0 - a0 b2, a0 b1 - a1 b0).
"""
import math


def box(pos, vel, size):
    return dict(x=float(pos[0]), y=float(pos[1]), z=float(pos[2]), Vx=float(vel[0]), Vy=float(vel[1]),
                x_width=float(size[0]), y_width=float(size[1]), z_width=float(size[2]))


class FakeDetector:
    """The members the getters read: obstacleMsg_, obstacleHist_, histSize_, colorDistance_ and
    the odometry (position and yaw)."""

    def __init__(self, hist_size, color_distance):
        self.hist_size = hist_size
        self.color_distance = color_distance
        self.obstacle_msg = []
        self.obstacle_hist = []
        self.robot_pos = [0.0, 0.0, 0.0]
        self.robot_yaw = 0.0

    def hist_cb(self):
        """:337-347"""
        if len(self.obstacle_hist) == 0:
            self.obstacle_hist = [[] for _ in self.obstacle_msg]
        for i in range(len(self.obstacle_msg)):
            if len(self.obstacle_hist[i]) >= self.hist_size:
                self.obstacle_hist[i].pop()
            self.obstacle_hist[i].insert(0, self.obstacle_msg[i])

    def is_obstacle_in_sensor_range(self, ob, fov):
        """:482-500"""
        p_robot = self.robot_pos
        p_obstacle = [ob["x"], ob["y"], ob["z"]]
        diff = [p_obstacle[0] - p_robot[0], p_obstacle[1] - p_robot[1], p_obstacle[2] - p_robot[2]]
        diff[2] = 0.0
        distance = math.sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2])
        yaw = self.robot_yaw
        direction = [math.cos(yaw), math.sin(yaw), 0.0]
        angle = angle_between_vectors(direction, diff)
        return angle <= fov / 2 and distance <= self.color_distance

    def get_obstacles_in_sensor_range(self, fov, robot_size):
        """:513-523 -- the boxes in range, in index order, widths + robotSize."""
        obstacles = []
        for ob in self.obstacle_msg:
            if self.is_obstacle_in_sensor_range(ob, fov):
                ob = dict(ob)
                ob["x_width"] += robot_size[0]
                ob["y_width"] += robot_size[1]
                ob["z_width"] += robot_size[2]
                obstacles.append(ob)
        return obstacles

    def get_dynamic_obstacles_hist(self, robot_size, fov=2 * math.pi):
        """:525-556 -- (posHist, velHist, sizeHist), one list of 3-vectors per obstacle whose newest
        history entry is in range (the reference's fov is 2 pi, :533; a parameter here so the gate's
        fov < 2 pi cases have a restatement too)."""
        pos_hist, vel_hist, size_hist = [], [], []
        if len(self.obstacle_hist):
            for i in range(len(self.obstacle_hist)):
                if len(self.obstacle_hist[i]) == 0:  # the reference indexes [0] of an empty deque
                    continue                           # (undefined); a track with no entry is out
                if self.is_obstacle_in_sensor_range(self.obstacle_hist[i][0], fov):
                    ob_pos, ob_vel, ob_size = [], [], []
                    for h in self.obstacle_hist[i]:
                        ob_pos.append([h["x"], h["y"], h["z"]])
                        ob_vel.append([h["Vx"], h["Vy"], 0.0])
                        ob_size.append([h["x_width"] + robot_size[0], h["y_width"] + robot_size[1],
                                        h["z_width"] + robot_size[2]])
                    pos_hist.append(ob_pos)
                    vel_hist.append(ob_vel)
                    size_hist.append(ob_size)
        return pos_hist, vel_hist, size_hist


def angle_between_vectors(a, b):
    """utils.h:58-60"""
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    return math.atan2(math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), a[0] * b[0] + a[1] * b[1] + a[2] * b[2])


def margins(robot_pos, robot_yaw, ob_pos, fov, color_distance):
    """(|distance - colorDistance_|, |angle - fov / 2|) of one pair: how far each comparison of :493
    is from flipping (the tests keep their seeded inputs away from the thresholds)."""
    d = [ob_pos[0] - robot_pos[0], ob_pos[1] - robot_pos[1], 0.0]
    dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    ang = angle_between_vectors([math.cos(robot_yaw), math.sin(robot_yaw), 0.0], d)
    return abs(dist - color_distance), abs(ang - fov / 2)


# ---------------------------------------------------------------- the library's outputs, restated
def gather(worlds_pushes, hist_size, color_distance, fov, robot_size, K, robot_pos, robot_yaw=None):
    """What impc_detect_gather_device writes (include/impc_detect.h), built from the getters above.
    worlds_pushes: per world, the pushes in time order, each (pos [M][3], vel [M][3], size [M][3]);
    one world serves every instance, else world i serves instance i.  Returns a dict of numpy arrays
    num, in_range [I], src, hist_len [I][K], pos_hist, vel_hist [I][K][H][3], cur_pos, cur_vel,
    cur_size [I][K][3], the empty slots as the header states them."""
    import numpy as np
    I, H = len(robot_pos), hist_size
    dets = []
    for pushes in worlds_pushes:
        det = FakeDetector(hist_size, color_distance)
        for pos, vel, size in pushes:
            det.obstacle_msg = [box(p, v, s) for p, v, s in zip(pos, vel, size)]
            det.hist_cb()
        dets.append(det)
    out = dict(num=np.zeros(I, np.int32), in_range=np.zeros(I, np.int32), src=np.full((I, K), -1, np.int32),
               hist_len=np.zeros((I, K), np.int32), pos_hist=np.zeros((I, K, H, 3)), vel_hist=np.zeros((I, K, H, 3)),
               cur_pos=np.zeros((I, K, 3)), cur_vel=np.zeros((I, K, 3)), cur_size=np.zeros((I, K, 3)))
    for i in range(I):
        det = dets[0] if len(dets) == 1 else dets[i]
        det.robot_pos = [float(v) for v in robot_pos[i]]
        det.robot_yaw = 0.0 if robot_yaw is None else float(robot_yaw[i])
        ph, vh, sh = det.get_dynamic_obstacles_hist(robot_size, fov)
        # the world index of every kept track: the same test, in the same order
        idx = [j for j, h in enumerate(det.obstacle_hist) if h and det.is_obstacle_in_sensor_range(h[0], fov)]
        assert len(idx) == len(ph)
        out["in_range"][i] = len(ph)
        out["num"][i] = min(len(ph), K)
        # the no-predictor getter sees the same boxes: after a push obstacleMsg_ is every history's entry 0
        if det.obstacle_hist and det.obstacle_hist[0]:
            cur = det.get_obstacles_in_sensor_range(fov, robot_size)
            assert len(cur) == len(ph)
        for s in range(out["num"][i]):
            n = len(ph[s])
            out["src"][i, s] = idx[s]
            out["hist_len"][i, s] = n
            out["pos_hist"][i, s, :n] = ph[s]
            out["vel_hist"][i, s, :n] = vh[s]
            out["cur_pos"][i, s] = ph[s][0]
            out["cur_vel"][i, s] = vh[s][0]
            out["cur_size"][i, s] = [cur[s]["x_width"], cur[s]["y_width"], cur[s]["z_width"]]
            assert out["cur_size"][i, s].tolist() == sh[s][0]
    return out
