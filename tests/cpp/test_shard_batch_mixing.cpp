// One rank of tests/test_gpu_batch_split.py::test_sharded_engine_refuses_a_batch_mixing_graph: SimpleInfer::ShardedEngine::Init on an engine whose
// graph holds an operator that combines images of the batch.  With WORLD_SIZE > 1 every rank's slab would be a piece of one batch, so Init
// returns kUnsupport -- before any rank waits for another; with WORLD_SIZE == 1 the engine is served, and the gathered tensor is written out.
//
// usage (RANK / WORLD_SIZE from the launcher): test_shard_batch_mixing group model.pnnx.param model.pnnx.bin input.f32 gathered.f32
// prints "rank R of W: mixing M init S forward S"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "engine.h"
#include "shard.h"
#include "si_hip.h"

using namespace SimpleInfer;

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const int rank = std::atoi(std::getenv("RANK") ? std::getenv("RANK") : "0");
    const int world = std::atoi(std::getenv("WORLD_SIZE") ? std::getenv("WORLD_SIZE") : "1");
    InitializeContext();
    Engine engine;
    if (engine.SetOption("outputs_to_host", 0) != Status::kSuccess || engine.LoadModel(argv[2], argv[3]) != Status::kSuccess) return 3;
    const std::string in_name = engine.InputNames()[0], out_name = engine.OutputNames()[0];
    std::vector<int> shape;
    if (engine.OperandShape(in_name, shape) != Status::kSuccess) return 3;
    Tensor in(DataType::kFloat32, shape, false);
    std::vector<float> x(in.NumElements());
    FILE* f = std::fopen(argv[4], "rb");
    if (!f || std::fread(x.data(), sizeof(float), x.size(), f) != x.size()) return 4;
    std::fclose(f);
    in.SetData(x.data());
    ShardedEngine sharded;
    const Status init = sharded.Init(argv[1], rank, world, &engine, out_name, 2, 20.0, GatherMode::kDirect);
    int forward = -1;
    if (init == Status::kSuccess) {
        Status s = engine.Input(in_name, in);
        if (s == Status::kSuccess) s = sharded.Forward();
        if (s == Status::kSuccess) s = sharded.Flush();
        Tensor gathered;
        if (s == Status::kSuccess) s = sharded.Gathered(gathered);
        if (s == Status::kSuccess) {
            std::vector<float> y(gathered.NumElements());
            if (si_hip_memcpy_d2h(y.data(), gathered.RawData(), y.size() * sizeof(float), nullptr) != 0 || si_hip_stream_sync(nullptr) != 0) return 5;
            FILE* g = std::fopen(argv[5], "wb");
            if (!g || std::fwrite(y.data(), sizeof(float), y.size(), g) != y.size()) return 5;
            std::fclose(g);
        }
        forward = static_cast<int>(s);
    }
    // (the launcher hands back rank 0's stdout only: every rank leaves its line in a file of its own too)
    char line[160];
    std::snprintf(line, sizeof(line), "rank %d of %d: mixing %zu init %d forward %d\n", rank, world, engine.BatchMixingLayers().size(),
                  static_cast<int>(init), forward);
    std::fputs(line, stdout);
    FILE* st = std::fopen((std::string(argv[5]) + ".rank" + std::to_string(rank)).c_str(), "w");
    if (!st) return 6;
    std::fputs(line, st);
    std::fclose(st);
    return 0;
}
