// A point and a direction on a drivable's polyline at a distance along it: the reference's two walks, restated to the bit
// (FP64, no contraction).  Shared by the replay writer and the pose columns of the vehicle rows (engine_host.cpp); the
// device restates them once more (cfx_kernels.h vehiclePose).  The two walks differ on purpose: the point moves on to the
// next segment while `dis > l`, the direction stops at the first segment with `remain < l`.
#pragma once

#include <cmath>
#include <vector>

#include "roadnet.h"

namespace cfa {

inline double segmentLength(Pt a, Pt b) {  // Point::len of the difference, utility.cpp:74-76
    const double dx = a.x - b.x, dy = a.y - b.y;
    return sqrt(dx * dx + dy * dy);
}

// getPointByDistance roadnet.cpp:17-29
inline Pt pointByDistance(const std::vector<Pt> &points, double dis) {
    double total = 0.0;
    for (size_t i = 0; i + 1 < points.size(); ++i) total += segmentLength(points[i + 1], points[i]);
    double lo = dis > 0 ? dis : 0;  // max2double(dis, 0)
    dis = lo < total ? lo : total;  // min2double(., length)
    if (dis <= 0.0) return points[0];
    for (size_t i = 1; i < points.size(); ++i) {
        double l = segmentLength(points[i - 1], points[i]);
        if (dis > l) dis -= l;
        else {
            const double k = dis / l;
            return {points[i - 1].x + (points[i].x - points[i - 1].x) * k, points[i - 1].y + (points[i].y - points[i - 1].y) * k};
        }
    }
    return points.back();
}

// Drivable::getDirectionByDistance roadnet.cpp:400-411: the unit vector (Point::unit utility.cpp:63-66) of the segment
inline Pt directionByDistance(const std::vector<Pt> &points, double dis) {
    auto unitOf = [&](size_t i) {
        const double dx = points[i + 1].x - points[i].x, dy = points[i + 1].y - points[i].y;
        const double l = sqrt(dx * dx + dy * dy);
        return Pt{dx / l, dy / l};
    };
    double remain = dis;
    for (int i = 0; i + 1 < (int) points.size(); ++i) {
        double l = segmentLength(points[i + 1], points[i]);
        if (remain < l) return unitOf((size_t) i);
        remain -= l;
    }
    return unitOf(points.size() - 2);
}

}  // namespace cfa
