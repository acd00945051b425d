// What LoopClosingStep::SearchAndFuseResident (facade/LoopClosingStep.h) touches beyond tests/cpp/mock_model_search_in_neighbors.h: the
// constructor and setter of Sophus::Sim3f that LoopClosing.cc:2042-2043 uses and tests/cpp/mock_sophus.h lacks.  TEST INFRASTRUCTURE.
#pragma once
#include "mock_model_search_in_neighbors.h"

struct Sim3fQ : Sophus::Sim3f {
    Sim3fQ() {}
    Sim3fQ(const Eigen::Matrix3f &R_, const Eigen::Vector3f &t_, float s_) : Sophus::Sim3f(R_, t_, s_) {}
    Sim3fQ(const Eigen::Quaternionf &q, const Eigen::Vector3f &t_) : Sophus::Sim3f(q.toRotationMatrix(), t_, 1.f) {}
    void setScale(float s_) { s = s_; }
};
