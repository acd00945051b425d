// Scalar restatement of ORB_SLAM3::KeyFrameDatabase (R/lib_src/KeyFrameDatabase.cc) and DBoW2's L1Scoring::score
// (R/Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the checker of librumi_hip's key-frame database (include/rumi_kfdb.h).
// Built by the tests with g++ -ffp-contract=off.  It reads a script on stdin, one command per line, and prints one line per query:
//   A id map n (word value)*n    add            E id          erase             M map     clearMap       C   clear
//   B map bad                    Map::IsBad     K id map      KeyFrame::GetMap  D id bad  KeyFrame::isBad
//   V id k c1 .. ck              GetBestCovisibilityKeyFrames(10) of id (ids not in the database are left out, as SetBadFlag removes them)
//   R qid map n (word value)*n                                   DetectRelocalizationCandidates
//   N qid map ncand nconn conn*nconn n (word value)*n            DetectNBestCandidates
// Values are C99 hex floats.  Output: "R qid | id:sibits .. | cand ..." and "N qid | id:sibits .. | loop .. | merge ..", si as the hex of
// its float bits, the scored pairs in lScoreAndMatch order.
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <list>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

typedef std::map<unsigned, double> BowVector;     // DBoW2::BowVector: std::map<WordId, WordValue>

struct KeyFrame {                                 // the fields of KeyFrame the database reads and writes
    uint64_t mnId = 0;
    BowVector mBowVec;
    int map = 0;
    bool bad = false;
    std::vector<KeyFrame *> covisibles;           // GetBestCovisibilityKeyFrames(10)
    uint64_t mnRelocQuery = 0;                    // KeyFrame.cc:188-189: the query ids start at 0
    int mnRelocWords = 0;
    float mRelocScore = 0;                        // left uninitialised by the reference; 0 here
    uint64_t mnPlaceRecognitionQuery = 0;
    int mnPlaceRecognitionWords = 0;
    float mPlaceRecognitionScore = 0;
};

static std::map<uint64_t, KeyFrame> g_kfs;        // key-frame objects outlive their stay in the inverted file
static std::map<unsigned, std::list<KeyFrame *>> g_inv;   // mvInvertedFile
static std::set<uint64_t> g_inDb;
static std::set<int> g_badMaps;

// ScoringObject.cpp:23-68
static double l1_score(const BowVector &v1, const BowVector &v2) {
    auto v1_it = v1.begin(), v2_it = v2.begin();
    double score = 0;
    while (v1_it != v1.end() && v2_it != v2.end()) {
        const double &vi = v1_it->second, &wi = v2_it->second;
        if (v1_it->first == v2_it->first) {
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++v1_it; ++v2_it;
        } else if (v1_it->first < v2_it->first) {
            v1_it = v1.lower_bound(v2_it->first);
        } else {
            v2_it = v2.lower_bound(v1_it->first);
        }
    }
    score = -score / 2.0;
    return score;
}

static void add(KeyFrame *k) {                                 // :38-44
    for (auto &kv : k->mBowVec) g_inv[kv.first].push_back(k);
    g_inDb.insert(k->mnId);
}
static void erase(KeyFrame *k) {                               // :46-64, then SetBadFlag drops the key-frame from every covisibility list
    for (auto &kv : k->mBowVec) {
        auto &l = g_inv[kv.first];
        for (auto it = l.begin(); it != l.end(); ++it) if (*it == k) { l.erase(it); break; }
    }
    g_inDb.erase(k->mnId);
    for (auto &p : g_kfs) {
        auto &c = p.second.covisibles;
        for (auto it = c.begin(); it != c.end();) it = *it == k ? c.erase(it) : it + 1;
    }
}

static std::string bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    char b[16];
    std::snprintf(b, sizeof b, "%08x", u);
    return b;
}

// :733-843
static std::string reloc(uint64_t qid, int qmap, const BowVector &bow) {
    std::ostringstream out;
    out << "R " << qid << " |";
    std::list<KeyFrame *> lKFsSharingWords;
    for (auto &kv : bow) {
        for (KeyFrame *k : g_inv[kv.first]) {
            if (k->mnRelocQuery != qid) { k->mnRelocWords = 0; k->mnRelocQuery = qid; lKFsSharingWords.push_back(k); }
            k->mnRelocWords++;
        }
    }
    std::vector<KeyFrame *> cand;
    if (!lKFsSharingWords.empty()) {
        int maxCommonWords = 0;
        for (KeyFrame *k : lKFsSharingWords) if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
        int minCommonWords = maxCommonWords * 0.8f;
        std::list<std::pair<float, KeyFrame *>> lScoreAndMatch;
        for (KeyFrame *k : lKFsSharingWords)
            if (k->mnRelocWords > minCommonWords) {
                float si = (float)l1_score(bow, k->mBowVec);
                k->mRelocScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, k));
            }
        for (auto &p : lScoreAndMatch) out << " " << p.second->mnId << ":" << bits(p.first);
        std::list<std::pair<float, KeyFrame *>> lAcc;
        float bestAccScore = 0;
        for (auto &p : lScoreAndMatch) {
            KeyFrame *k = p.second;
            float bestScore = p.first, accScore = bestScore;
            KeyFrame *pBestKF = k;
            for (KeyFrame *k2 : k->covisibles) {
                if (k2->mnRelocQuery != qid) continue;
                accScore += k2->mRelocScore;
                if (k2->mRelocScore > bestScore) { pBestKF = k2; bestScore = k2->mRelocScore; }
            }
            lAcc.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        float minScoreToRetain = 0.75f * bestAccScore;
        std::set<KeyFrame *> spAlreadyAddedKF;
        for (auto &p : lAcc) {
            if (p.first > minScoreToRetain) {
                KeyFrame *k = p.second;
                if (k->map != qmap) continue;
                if (!spAlreadyAddedKF.count(k)) { cand.push_back(k); spAlreadyAddedKF.insert(k); }
            }
        }
    }
    out << " |";
    for (KeyFrame *k : cand) out << " " << k->mnId;
    return out.str();
}

// :604-708
static std::string nbest(uint64_t qid, int qmap, int N, const std::set<uint64_t> &connected, const BowVector &bow) {
    std::ostringstream out;
    out << "N " << qid << " |";
    std::list<KeyFrame *> lKFsSharingWords;
    for (auto &kv : bow) {
        for (KeyFrame *k : g_inv[kv.first]) {
            if (k->mnPlaceRecognitionQuery != qid) {
                k->mnPlaceRecognitionWords = 0;
                if (!connected.count(k->mnId)) { k->mnPlaceRecognitionQuery = qid; lKFsSharingWords.push_back(k); }
            }
            k->mnPlaceRecognitionWords++;
        }
    }
    std::vector<KeyFrame *> loop, merge;
    if (!lKFsSharingWords.empty()) {
        int maxCommonWords = 0;
        for (KeyFrame *k : lKFsSharingWords) if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;
        int minCommonWords = maxCommonWords * 0.8f;
        std::list<std::pair<float, KeyFrame *>> lScoreAndMatch;
        for (KeyFrame *k : lKFsSharingWords)
            if (k->mnPlaceRecognitionWords > minCommonWords) {
                float si = (float)l1_score(bow, k->mBowVec);
                k->mPlaceRecognitionScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, k));
            }
        for (auto &p : lScoreAndMatch) out << " " << p.second->mnId << ":" << bits(p.first);
        std::list<std::pair<float, KeyFrame *>> lAcc;
        for (auto &p : lScoreAndMatch) {
            KeyFrame *k = p.second;
            float bestScore = p.first, accScore = bestScore;
            KeyFrame *pBestKF = k;
            for (KeyFrame *k2 : k->covisibles) {
                if (k2->mnPlaceRecognitionQuery != qid) continue;
                accScore += k2->mPlaceRecognitionScore;
                if (k2->mPlaceRecognitionScore > bestScore) { pBestKF = k2; bestScore = k2->mPlaceRecognitionScore; }
            }
            lAcc.push_back(std::make_pair(accScore, pBestKF));
        }
        lAcc.sort([](const std::pair<float, KeyFrame *> &a, const std::pair<float, KeyFrame *> &b) { return a.first > b.first; });   // compFirst
        std::set<KeyFrame *> spAlreadyAddedKF;
        size_t i = 0;
        auto it = lAcc.begin();
        while (i < lAcc.size() && ((int)loop.size() < N || (int)merge.size() < N)) {
            KeyFrame *k = it->second;
            if (k->bad) { i++; it++; continue; }      // the reference's `continue` here never advances; the database skips and advances
            if (!spAlreadyAddedKF.count(k)) {
                if (qmap == k->map && (int)loop.size() < N) loop.push_back(k);
                else if (qmap != k->map && (int)merge.size() < N && !g_badMaps.count(k->map)) merge.push_back(k);
                spAlreadyAddedKF.insert(k);
            }
            i++; it++;
        }
    }
    out << " |";
    for (KeyFrame *k : loop) out << " " << k->mnId;
    out << " |";
    for (KeyFrame *k : merge) out << " " << k->mnId;
    return out.str();
}

static BowVector read_bow(std::istringstream &in) {
    int n;
    in >> n;
    BowVector b;
    for (int j = 0; j < n; j++) {
        unsigned w;
        std::string v;
        in >> w >> v;
        b[w] = std::strtod(v.c_str(), nullptr);
    }
    return b;
}

int main() {
    // KFDB_ORACLE_TIMING=1: the time of each query function call alone (not the parsing of the script) goes to stderr, one line per query
    const bool timing = std::getenv("KFDB_ORACLE_TIMING") != nullptr;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "A") {
            uint64_t id; int map;
            in >> id >> map;
            KeyFrame &k = g_kfs[id];
            k.mnId = id; k.map = map; k.mBowVec = read_bow(in); k.bad = false;
            k.covisibles.clear();                                 // the caller sets them (V) after the add
            add(&k);
        } else if (op == "E") {
            uint64_t id; in >> id;
            if (g_inDb.count(id)) erase(&g_kfs[id]);
        } else if (op == "M") {                                   // :66-94, by each key-frame's current map
            int map; in >> map;
            std::vector<KeyFrame *> gone;
            for (uint64_t id : g_inDb) if (g_kfs[id].map == map) gone.push_back(&g_kfs[id]);
            for (KeyFrame *k : gone) erase(k);
        } else if (op == "C") {
            std::vector<KeyFrame *> gone;
            for (uint64_t id : g_inDb) gone.push_back(&g_kfs[id]);
            for (KeyFrame *k : gone) erase(k);
        } else if (op == "B") {
            int map, bad; in >> map >> bad;
            if (bad) g_badMaps.insert(map); else g_badMaps.erase(map);
        } else if (op == "K") {
            uint64_t id; int map; in >> id >> map;
            if (g_inDb.count(id)) g_kfs[id].map = map;
        } else if (op == "D") {
            uint64_t id; int bad; in >> id >> bad;
            if (g_inDb.count(id)) g_kfs[id].bad = bad != 0;
        } else if (op == "V") {
            uint64_t id; int n; in >> id >> n;
            std::vector<KeyFrame *> c;
            for (int j = 0; j < n; j++) { int64_t x; in >> x; if (x >= 0 && g_inDb.count((uint64_t)x)) c.push_back(&g_kfs[(uint64_t)x]); }
            if (g_inDb.count(id)) g_kfs[id].covisibles = c;
        } else if (op == "R") {
            uint64_t qid; int map; in >> qid >> map;
            BowVector b = read_bow(in);
            const auto t0 = std::chrono::steady_clock::now();
            std::string r = reloc(qid, map, b);
            if (timing) std::fprintf(stderr, "query_ms %.6f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            std::cout << r << "\n";
        } else if (op == "N") {
            uint64_t qid; int map, N, nc; in >> qid >> map >> N >> nc;
            std::set<uint64_t> conn;
            for (int j = 0; j < nc; j++) { uint64_t c; in >> c; conn.insert(c); }
            BowVector b = read_bow(in);
            const auto t0 = std::chrono::steady_clock::now();
            std::string r = nbest(qid, map, N, conn, b);
            if (timing) std::fprintf(stderr, "query_ms %.6f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            std::cout << r << "\n";
        } else {
            std::cerr << "kfdb_oracle: unknown command " << op << "\n";
            return 2;
        }
    }
    return 0;
}
