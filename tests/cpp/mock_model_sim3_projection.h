// What LoopClosingStep::SearchByProjectionResident / CovisibleCheckResident (facade/LoopClosingStep.h) touch beyond
// tests/cpp/mock_model_search_and_fuse.h: Converter::toSophus(g2o::Sim3) (Converter.cc:291-294) over the stand-ins of tests/cpp/mock_sophus.h.
// TEST INFRASTRUCTURE.
#pragma once
#include "mock_model_search_and_fuse.h"

inline Sophus::Sim3f toSophusMock(const g2o::Sim3 &S) {
    const Eigen::Quaterniond q = S.rotation();
    const Eigen::Quaternionf qf((float)q.w(), (float)q.x(), (float)q.y(), (float)q.z());
    const Eigen::Vector3d t = S.translation();
    return Sophus::Sim3f(qf.toRotationMatrix(), Eigen::Vector3f((float)t(0), (float)t(1), (float)t(2)), (float)S.scale());
}
